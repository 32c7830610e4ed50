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
