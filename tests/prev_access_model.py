"""The judge of nx_trace_prev_access: a sequential dictionary model.  It walks every access in the stated time order — (epoch, natural
trace row, index of the stream) — over one dict, exactly as the reference's RegisterMemCheckSideNote::access and
ReadWriteMemCheckSideNote::last_access.insert do, and reads the final-state tables off the dict at the end.  Shared by
tests/test_prev_access_cpu.py and tests/test_gpu_prev_access.py; all comparisons against it are exact word equalities."""
import numpy as np

P = (1 << 31) - 1


def _bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def coset_row_of_pos(pos, log_size):
    """natural coset row of a storage position of a column in bit-reversed circle-domain order: the circle domain holds the even rows in
    its first half and the odd rows, backwards, in its second"""
    n, d = 1 << log_size, _bitrev(pos, log_size)
    return 2 * d if d < n // 2 else 2 * (n - 1 - d) + 1


def rows_of_positions(log_size, linear):
    n = 1 << log_size
    return np.arange(n, dtype=np.int64) if linear else np.array([coset_row_of_pos(p, log_size) for p in range(n)], dtype=np.int64)


def to_storage(natural, log_size):
    """a column given in natural row order -> bit-reversed circle-domain order"""
    natural = np.asarray(natural)
    return natural[rows_of_positions(log_size, False)]


def two_linear_streams(rng, log_size):
    """one epoch: a linear stream of 2^log_size rows with flags and one of 2 rows without, key entries of 8 and 5 bits, one payload
    column, every output wanted.  At 2^20 rows a block of the sort takes five tiles, one more than the minimum."""
    streams = []
    for log, flags in ((log_size, True), (1, False)):
        n = 1 << log
        streams.append({"key": [rng.integers(0, 256, n, dtype=np.uint32), rng.integers(0, 32, n, dtype=np.uint32)],
                        "flag": rng.integers(0, 3, n, dtype=np.uint32) * rng.integers(1, 9, n, dtype=np.uint32) if flags else None,
                        "payload": [rng.integers(0, P, n, dtype=np.uint32)], "log_size": log, "epoch": 0, "linear": True, "prev_wanted": [True], "want_ord": True})
    return streams


def model_by_sorting(streams, key_bits, n_payload, init=None):
    """What model() returns, for sizes its Python walk is too slow for, from the definition in array form: the accepted accesses in time
    order (epoch, natural row, stream), numpy's stable sort by key, then every element takes the payload of the one before it in its
    run (init at the head) and its place in the run.  tests/test_prev_access_cpu.py holds it to model()."""
    init = np.zeros(n_payload, np.uint32) if init is None else np.asarray(init, np.uint32)
    epoch, row, sid, key, use, oor_at, pay = [], [], [], [], [], [], [[] for _ in range(n_payload)]
    for s, st in enumerate(streams):
        n = 1 << st["log_size"]
        k, oor, shift = np.zeros(n, np.uint64), np.zeros(n, bool), 0
        for col, b in zip(st["key"], key_bits):
            x = np.asarray(col).astype(np.uint64)
            oor |= x >= np.uint64(1 << b)
            k |= x << np.uint64(shift)
            shift += b
        acc = np.ones(n, bool) if st.get("flag") is None else np.asarray(st["flag"]) != 0
        epoch.append(np.full(n, int(st.get("epoch", 0)), np.int64))
        row.append(rows_of_positions(st["log_size"], st.get("linear", False)))
        sid.append(np.full(n, s, np.int64))
        key.append(k)
        use.append(acc & ~oor)
        oor_at += [(s, int(p)) for p in np.flatnonzero(acc & oor)[:1]]
        p = st.get("payload") or [None] * n_payload
        for c in range(n_payload):
            pay[c].append(np.zeros(n, np.uint32) if p[c] is None else np.asarray(p[c], np.uint32))
    epoch, row, sid, key, use = (np.concatenate(a) for a in (epoch, row, sid, key, use))
    pay = [np.concatenate(a) for a in pay]
    t = np.lexsort((sid, row, epoch))                       # time order: the last key is the first criterion
    t = t[use[t]]
    o = t[np.argsort(key[t], kind="stable")]                # by key, in time order inside a key
    ks, m = key[o], len(o)
    head, tail = np.ones(m, bool), np.ones(m, bool)
    head[1:] = ks[1:] != ks[:-1]
    tail[:-1] = head[1:]
    at = np.arange(m, dtype=np.int64)
    place = at - np.maximum.accumulate(np.where(head, at, 0))
    ends = np.cumsum([0] + [1 << st["log_size"] for st in streams])
    cut = lambda a: [a[ends[s]:ends[s + 1]] for s in range(len(streams))]
    prev = []
    for c in range(n_payload):
        moved, out = pay[c][o], np.zeros(len(key), np.uint32)
        out[o] = np.where(head, init[c], np.concatenate([moved[:1], moved[:-1]]))
        prev.append(cut(out))
    ordinal = np.zeros(len(key), np.uint32)
    ordinal[o] = place
    return {"prev": [[prev[c][s] for c in range(n_payload)] for s in range(len(streams))], "ordinal": cut(ordinal), "keys": ks[head].astype(np.uint32),
            "counts": (place[tail] + 1).astype(np.uint32), "last": [pay[c][o][tail] for c in range(n_payload)], "bad": min(oor_at) if oor_at else None}


def model(streams, key_bits, n_payload, init=None):
    """streams: dicts of HOST arrays in storage order — key: one array per key column; log_size; optional flag (None: every row
    accesses), payload (n_payload arrays, None entries read as 0), epoch, linear.  Returns a dict: prev[s][c] / ordinal[s]: the
    expected output columns (0 on rows that do not access); keys / counts / last[c]: the summary in ascending key order; bad: the
    smallest (stream, position) of an accessing row with an entry outside its key_bits, or None (such rows are skipped)."""
    init = [0] * n_payload if init is None else [int(x) for x in init]
    order = []
    for s, st in enumerate(streams):
        rows = rows_of_positions(st["log_size"], st.get("linear", False))
        order += [(int(st.get("epoch", 0)), int(r), s, pos) for pos, r in enumerate(rows)]
    order.sort()
    prev = [[np.zeros(1 << st["log_size"], np.uint32) for _ in range(n_payload)] for st in streams]
    ordinal = [np.zeros(1 << st["log_size"], np.uint32) for st in streams]
    last, bad = {}, None
    for _, _, s, pos in order:
        st = streams[s]
        if st.get("flag") is not None and int(st["flag"][pos]) == 0:
            continue
        key, shift, oor = 0, 0, False
        for col, b in zip(st["key"], key_bits):
            x = int(col[pos])
            oor |= x >= (1 << b)
            key |= x << shift
            shift += b
        if oor:
            bad = (s, pos) if bad is None else min(bad, (s, pos))
            continue
        before, count = last.get(key, (init, 0))
        for c in range(n_payload):
            prev[s][c][pos] = before[c]
        ordinal[s][pos] = count
        pay = st.get("payload") or [None] * n_payload
        last[key] = ([0 if pay[c] is None else int(pay[c][pos]) for c in range(n_payload)], count + 1)
    keys = sorted(last)
    return {"prev": prev, "ordinal": ordinal, "keys": np.array(keys, np.uint32), "counts": np.array([last[k][1] for k in keys], np.uint32),
            "last": [np.array([last[k][0][c] for k in keys], np.uint32) for c in range(n_payload)], "bad": bad}
