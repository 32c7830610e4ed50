"""The judge of nx_trace_access_chain: a sequential dictionary walk in plain Python integers.  It visits every access in the stated
time order — (epoch, natural row, index of the stream, sub-access) — over one dict.  An access reads the state of its key (init when
untouched) and the number of earlier accesses, then leaves its own payload word (GIVEN: the load/store chip's
last_access.insert(addr, (clk, value)), prover/src/chips/instructions/i/load_store.rs:199-205) or what it found plus delta modulo 2^32
(ADD: KeccakChip::update_state_timestamps, prover/src/chips/custom.rs:107-123, which reports the timestamp of each of 200 bytes and
leaves ts + 1 beside the output byte).

Streams are dicts of HOST arrays.  A column stream is that of tests/prev_access_model.py (key, flag, payload, log_size, epoch, linear)
with optional rule / delta lists.  A block stream has row (n_records ascending natural rows), span, key (one array of n_records words
per key column), flag (n_records words or None) and payload: per column None or n_records * span element values, record-major
(bytes as values below 256: the CHAIN_BYTES bit of a rule is a matter of device layout, which the model does not see).
model_by_sorting is the same answer in array form for the larger device cases; tests/test_access_chain_cpu.py holds it to the walk."""
import numpy as np

from prev_access_model import P, rows_of_positions

GIVEN, ADD, BYTES = 0, 1, 2
MASK32 = (1 << 32) - 1
BAD_ENTRY, BAD_SUB, BAD_ORDER, BAD_ROW = 0, 1, 2, 3          # "bad": (stream, position or record, sub-access, kind), the smallest


def is_block(st):
    return st.get("row") is not None


def n_units(st):
    return len(st["row"]) if is_block(st) else 1 << st["log_size"]


def n_elems(st):
    return len(st["row"]) * st["span"] if is_block(st) else 1 << st["log_size"]


def _rules(st, n_payload):
    rule = [GIVEN] * n_payload if st.get("rule") is None else [int(r) for r in st["rule"]]
    delta = [1] * n_payload if st.get("delta") is None else [int(d) & MASK32 for d in st["delta"]]
    return rule, delta


def _row_faults(streams):
    bad = []
    for s, st in enumerate(streams):
        if is_block(st):
            rows = [int(r) for r in st["row"]]
            bad += [(s, j, 0, BAD_ROW) for j, r in enumerate(rows) if r >> 31]
            bad += [(s, j, 0, BAD_ORDER) for j in range(1, len(rows)) if rows[j] <= rows[j - 1] and not rows[j] >> 31]
    return bad


def model(streams, key_bits, n_payload, init=None):
    """-> prev[s][c] / ordinal[s] / left[s][c] / key[s]: per element of stream s what the access found, how many came before it, what it
    left and its packed key (0 where it does not access); keys / counts / last[c]: the summary in ascending key order; bad."""
    init = [0] * n_payload if init is None else [int(x) for x in init]
    total_bits = sum(key_bits)
    order = []
    for s, st in enumerate(streams):
        if is_block(st):
            order += [(int(st.get("epoch", 0)), int(r), s, i, j) for j, r in enumerate(st["row"]) for i in range(st["span"])]
        else:
            order += [(int(st.get("epoch", 0)), int(r), s, 0, pos) for pos, r in enumerate(rows_of_positions(st["log_size"], st.get("linear", False)))]
    order.sort()
    prev = [[np.zeros(n_elems(st), np.uint32) for _ in range(n_payload)] for st in streams]
    left = [[np.zeros(n_elems(st), np.uint32) for _ in range(n_payload)] for st in streams]
    ordinal = [np.zeros(n_elems(st), np.uint32) for st in streams]
    keyof = [np.zeros(n_elems(st), np.uint32) for st in streams]
    rules = [_rules(st, n_payload) for st in streams]
    state, bad = {}, _row_faults(streams)
    for _, _, s, sub, unit in order:
        st = streams[s]
        if st.get("flag") is not None and int(st["flag"][unit]) == 0:
            continue
        key, shift, oor = 0, 0, False
        for col, b in zip(st["key"], key_bits):
            x = int(col[unit])
            oor |= x >= (1 << b)
            key |= x << shift
            shift += b
        if oor:
            bad.append((s, unit, 0, BAD_ENTRY))
            continue
        key += sub
        if key >> total_bits:
            bad.append((s, unit, sub, BAD_SUB))
            continue
        el = unit * st["span"] + sub if is_block(st) else unit
        before, count = state.get(key, (init, 0))
        pay = st.get("payload") or [None] * n_payload
        rule, delta = rules[s]
        after = []
        for c in range(n_payload):
            prev[s][c][el] = before[c]
            after.append((before[c] + delta[c]) & MASK32 if rule[c] & ADD else (0 if pay[c] is None else int(pay[c][el])))
            left[s][c][el] = after[c]
        ordinal[s][el], keyof[s][el] = count, key
        state[key] = (after, count + 1)
    keys = sorted(state)
    return {"prev": prev, "ordinal": ordinal, "left": left, "key": keyof, "keys": np.array(keys, np.uint32), "counts": np.array([state[k][1] for k in keys], np.uint32),
            "last": [np.array([state[k][0][c] for k in keys], np.uint32) for c in range(n_payload)], "bad": min(bad) if bad else None}


def model_by_sorting(streams, key_bits, n_payload, init=None):
    """What model() returns, from the definition in array form: the accepted accesses in time order, numpy's stable sort by key, and per
    column the state after element i of the sorted list = (value of the latest SET at or before i) + (the ADDs since), where the head
    of a run is the SET of init followed by its own op."""
    init = np.zeros(n_payload, np.uint64) if init is None else np.asarray(init, np.uint64)
    total_bits = sum(key_bits)
    epoch, row, sid, sub, key, use, faults = [], [], [], [], [], [], _row_faults(streams)
    adds, vals = [[] for _ in range(n_payload)], [[] for _ in range(n_payload)]
    for s, st in enumerate(streams):
        units, span = n_units(st), st["span"] if is_block(st) else 1
        k, oor, shift = np.zeros(units, np.uint64), np.zeros(units, bool), 0
        for col, b in zip(st["key"], key_bits):
            x = np.asarray(col).astype(np.uint64)
            oor |= x >= np.uint64(1 << b)
            k |= (x << np.uint64(shift)) & np.uint64(MASK32)
            shift += b
        acc = np.ones(units, bool) if st.get("flag") is None else np.asarray(st["flag"]) != 0
        r = np.asarray(st["row"], np.int64) if is_block(st) else rows_of_positions(st["log_size"], st.get("linear", False))
        k, oor, acc, r = (np.repeat(a, span) for a in (k, oor, acc, r))
        i = np.tile(np.arange(span, dtype=np.int64), units)
        k = k + i.astype(np.uint64)
        over = (k >> np.uint64(total_bits)) != 0
        n = units * span
        epoch.append(np.full(n, int(st.get("epoch", 0)), np.int64)); row.append(r); sid.append(np.full(n, s, np.int64)); sub.append(i); key.append(k)
        use.append(acc & ~oor & ~over)
        faults += [(s, int(e) // span, 0, BAD_ENTRY) for e in np.flatnonzero(acc & oor)[:1]]
        faults += [(s, int(e) // span, int(e) % span, BAD_SUB) for e in np.flatnonzero(acc & ~oor & over)[:1]]
        pay = st.get("payload") or [None] * n_payload
        rule, delta = _rules(st, n_payload)
        for c in range(n_payload):
            adds[c].append(np.full(n, bool(rule[c] & ADD)))
            vals[c].append(np.full(n, delta[c], np.uint64) if rule[c] & ADD else (np.zeros(n, np.uint64) if pay[c] is None else np.asarray(pay[c]).astype(np.uint64)))
    epoch, row, sid, sub, key, use = (np.concatenate(a) for a in (epoch, row, sid, sub, key, use))
    t = np.lexsort((sub, sid, row, epoch))
    t = t[use[t]]
    o = t[np.argsort(key[t], kind="stable")]
    ks, m = key[o], len(o)
    head, tail = np.ones(m, bool), np.ones(m, bool)
    head[1:] = ks[1:] != ks[:-1]
    tail[:-1] = head[1:]
    at = np.arange(m, dtype=np.int64)
    place = at - np.maximum.accumulate(np.where(head, at, 0)) if m else at
    ends = np.cumsum([0] + [n_elems(st) for st in streams])
    cut = lambda a: [a[ends[s]:ends[s + 1]] for s in range(len(streams))]
    prev, left, last = [], [], []
    for c in range(n_payload):
        is_add, v = np.concatenate(adds[c])[o], np.concatenate(vals[c])[o]
        is_set = head | ~is_add
        set_val = np.where(head & is_add, init[c] + v, v) & np.uint64(MASK32)
        grow = np.cumsum(np.where(is_set, np.uint64(0), v), dtype=np.uint64)
        since = np.maximum.accumulate(np.where(is_set, at, 0)) if m else at
        after = (set_val[since] + grow - grow[since]) & np.uint64(MASK32)
        before = np.where(head, init[c], np.concatenate([after[:1], after[:-1]]))
        p, l = np.zeros(len(key), np.uint32), np.zeros(len(key), np.uint32)
        p[o], l[o] = before.astype(np.uint32), after.astype(np.uint32)
        prev.append(cut(p)); left.append(cut(l)); last.append(after[tail].astype(np.uint32))
    ordinal, keyof = np.zeros(len(key), np.uint32), np.zeros(len(key), np.uint32)
    ordinal[o], keyof[o] = place, ks.astype(np.uint32)
    n_s = len(streams)
    return {"prev": [[prev[c][s] for c in range(n_payload)] for s in range(n_s)], "ordinal": cut(ordinal), "left": [[left[c][s] for c in range(n_payload)] for s in range(n_s)],
            "key": cut(keyof), "keys": ks[head].astype(np.uint32), "counts": (place[tail] + 1).astype(np.uint32), "last": last, "bad": min(faults) if faults else None}


def same_answers(a, b):
    assert a["bad"] == b["bad"], (a["bad"], b["bad"])
    for name in ("keys", "counts"):
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name
    assert len(a["last"]) == len(b["last"]) and all(np.array_equal(x, y) for x, y in zip(a["last"], b["last"])), "last"
    assert len(a["prev"]) == len(b["prev"])
    for s in range(len(a["prev"])):
        assert np.array_equal(a["ordinal"][s], b["ordinal"][s]) and np.array_equal(a["key"][s], b["key"][s]), s
        for name in ("prev", "left"):
            assert len(a[name][s]) == len(b[name][s]) and all(np.array_equal(x, y) for x, y in zip(a[name][s], b[name][s])), (name, s)


# ------------------------------------------------------------------------------------------------ builders shared by the suites ----
def column_stream(rng, key_bits, log_size, n_payload, keys, rule=None, delta=None, flags=False, null_payload=(), epoch=0, linear=False, prev_wanted=True, want_ord=True):
    """keys: packed keys in STORAGE order.  Payload words are raw 32-bit draws."""
    n = 1 << log_size
    rule = [GIVEN] * n_payload if rule is None else list(rule)
    cols, shift = [], 0
    for b in key_bits:
        cols.append(((np.asarray(keys, np.uint64) >> np.uint64(shift)) & np.uint64((1 << b) - 1)).astype(np.uint32))
        shift += b
    return {"key": cols, "flag": (rng.integers(0, 3, n, dtype=np.uint32) * rng.integers(1, 9, n, dtype=np.uint32)) if flags is True else (None if flags is False else flags),
            "payload": [None if (rule[c] & ADD or c in null_payload) else rng.integers(0, 1 << 32, n, dtype=np.uint32) for c in range(n_payload)],
            "rule": rule, "delta": delta, "log_size": log_size, "epoch": epoch, "linear": linear,
            "prev_wanted": ([True] * n_payload if prev_wanted is True else prev_wanted), "want_ord": want_ord}


def block_stream(rng, key_bits, rows, span, n_payload, keys, rule=None, delta=None, flags=False, null_payload=(), epoch=0, prev_wanted=True, want_ord=True):
    """keys: the packed key of sub-access 0 of every record.  A CHAIN_BYTES column draws bytes."""
    n_rec = len(rows)
    rule = [GIVEN] * n_payload if rule is None else list(rule)
    cols, shift = [], 0
    for b in key_bits:
        cols.append(((np.asarray(keys, np.uint64) >> np.uint64(shift)) & np.uint64((1 << b) - 1)).astype(np.uint32).reshape(n_rec))
        shift += b
    return {"row": np.asarray(rows, np.uint32).reshape(n_rec), "span": span, "key": cols,
            "flag": rng.integers(0, 3, n_rec, dtype=np.uint32) if flags is True else (None if flags is False else flags),
            "payload": [None if (rule[c] & ADD or c in null_payload) else rng.integers(0, 256 if rule[c] & BYTES else 1 << 32, n_rec * span, dtype=np.uint32) for c in range(n_payload)],
            "rule": rule, "delta": delta, "epoch": epoch, "prev_wanted": ([True] * n_payload if prev_wanted is True else prev_wanted), "want_ord": want_ord}


def keccak_ram_history(rng, log_size=6, out_bytes=None):
    """The RAM of a keccak guest on a 2^log_size-row main trace, key = the 32-bit address as [16, 16], payload (timestamp, value):
    an image (epoch 0, linear), the four byte streams of the load/store chip (epoch 1, timestamp row + 1, GIVEN) and one block stream of
    5 keccak records (span 200, timestamp ADD 1, value GIVEN | BYTES): buffer A hashed three times in a row, buffer B, which overlaps A
    by 8 bytes, twice.  Loads and stores touch both buffers before, between and after the records.  out_bytes: the 5 x 200 bytes the
    records leave (default: random; the device case passes keccak-f of what the records find).  -> (streams, rows, addresses)"""
    n = 1 << log_size
    key_bits, a_addr, b_addr = [16, 16], 0x1FF80, 0x1FF80 + 192
    image_addr = a_addr - 32 + np.arange(256, dtype=np.uint64)          # covers the start of A, not its end nor B's
    image = column_stream(rng, key_bits, 8, 2, image_addr, null_payload=(0,), epoch=0, linear=True, prev_wanted=None, want_ord=False)
    image["payload"][1] = rng.integers(0, 256, 256, dtype=np.uint32)
    rec_rows = np.array([n // 4, n // 4 + 1, n // 4 + 2, n // 2 + 3, n - 1], np.uint32)
    rec_addr = np.array([a_addr, a_addr, a_addr, b_addr, b_addr], np.uint64)
    nat = np.arange(n, dtype=np.int64)
    streams = [image]
    for lane in range(4):
        addr = (a_addr - 40 + rng.integers(0, 480, n)).astype(np.uint64)
        flag = (rng.integers(0, 4, n) != 0).astype(np.uint32)
        st = column_stream(rng, key_bits, log_size, 2, addr[rows_of_positions(log_size, False)], epoch=1, flags=flag[rows_of_positions(log_size, False)])
        st["payload"][0] = (nat + 1).astype(np.uint32)[rows_of_positions(log_size, False)]
        st["payload"][1] = rng.integers(0, 256, n, dtype=np.uint32)
        streams.append(st)
    kec = block_stream(rng, key_bits, rec_rows, 200, 2, rec_addr, rule=[ADD, GIVEN | BYTES], delta=[1, 0], epoch=1)
    if out_bytes is not None:
        kec["payload"][1] = np.asarray(out_bytes, np.uint32).reshape(-1)
    streams.append(kec)
    return streams, rec_rows, rec_addr.astype(np.uint32)
