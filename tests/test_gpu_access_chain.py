"""nx_trace_access_chain on the device against the sequential walk of tests/access_chain_model.py (its array twin for the larger
cases).  Every comparison is an equality of words; every buffer lies in a slab of guard words.
1. compatibility with nx_trace_prev_access;  2. chains across every boundary of the scan;  3. block streams;  4. placement;
5. refusals through a live context;  6. determinism and memory;  7. the RAM of a keccak guest end to end on the device: keccak-f by
nx_trace_keccak_round, the chain, nx_trace_keccak_memory_check fed the chain's output where it lies;  8. the closed keccak statement of
tests/keccak_memcheck_air.py with timestamps from the chain: checked, balanced, proved and verified."""
import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import access_chain_model as M
import keccak_memcheck_model as MM
import prev_access_model as PM

pytestmark = pytest.mark.gpu
P = M.P
NX_OK, NX_ERR_PROTOCOL = 0, -4
GUARD = 0xDEADBEEF
GIVEN, ADD, BYTES = M.GIVEN, M.ADD, M.BYTES


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


class Buf:
    """words at word offset `off` of a slab of guard words"""

    def __init__(self, be, nz, words, off=0):
        self.words = np.ascontiguousarray(words, np.uint32).reshape(-1)
        self.off, self.n = off, len(self.words)
        log = max(1, int(self.n + off + 4 - 1).bit_length())
        self.host = np.full(1 << log, GUARD, np.uint32)
        self.host[off:off + self.n] = self.words
        self.dev = nz.DeviceColumns(be, 1, log).upload(self.host[None, :])
        self.ptr = self.dev.ptr.value + 4 * off

    def read(self):
        """the words, after a look at the guards around them"""
        got = self.dev.to_cpu().reshape(-1)
        assert (got[:self.off] == GUARD).all() and (got[self.off + self.n:] == GUARD).all(), "guard words were written"
        return got[self.off:self.off + self.n]

    def untouched(self):
        return np.array_equal(self.dev.to_cpu().reshape(-1), self.host)


def pack_bytes(values):
    return np.ascontiguousarray(values, np.uint32).astype(np.uint8).view("<u4")


class Device:
    """the streams on the device: inputs uploaded, outputs filled with the guard word.  payload_ptrs: {(stream, column): device address}
    for a payload that already lies on the device"""

    def __init__(self, be, nz, streams, n_payload, cap=None, off=0, payload_ptrs=None):
        self.be, self.nz, self.streams, self.np, self.args, self.ins, self.out = be, nz, streams, n_payload, [], [], []
        put = lambda words: Buf(be, nz, words, off)
        for s, st in enumerate(streams):
            n, rule = M.n_elems(st), st.get("rule") or [GIVEN] * n_payload
            keys = [put(k) for k in st["key"]]
            flag = put(st["flag"]) if st.get("flag") is not None else None
            row = put(st["row"]) if M.is_block(st) else None
            pay = []
            for c, p in enumerate(st.get("payload") or [None] * n_payload):
                pay.append(None if p is None or (payload_ptrs and (s, c) in payload_ptrs) else put(pack_bytes(p) if rule[c] & BYTES else p))
            wanted = st.get("prev_wanted", [True] * n_payload)
            prev = None if wanted is None else [put(np.full(n, GUARD, np.uint32)) if w else None for w in wanted]
            ordinal = put(np.full(n, GUARD, np.uint32)) if st.get("want_ord", True) else None
            self.ins += keys + [b for b in [flag, row] + pay if b is not None]
            arg = {"key": [k.ptr for k in keys], "flag": flag.ptr if flag else None, "row": row.ptr if row else None,
                   "payload": [(payload_ptrs or {}).get((s, c)) or (b.ptr if b else None) for c, b in enumerate(pay)], "rule": st.get("rule"), "delta": st.get("delta"),
                   "prev": [b.ptr if b else None for b in prev] if prev is not None else None, "ordinal": ordinal.ptr if ordinal else None,
                   "epoch": st.get("epoch", 0), "linear": st.get("linear", False)}
            arg.update({"n_records": len(st["row"]), "span": st["span"]} if M.is_block(st) else {"log_size": st["log_size"]})
            if arg["payload"] == [None] * n_payload and s % 2:
                arg["payload"] = None                          # a NULL table is a table of NULLs
            self.args.append(arg)
            self.out.append((prev, ordinal))
        self.cap, self.summary, self.sums = cap, None, None
        if cap is not None:
            self.sums = [Buf(be, nz, np.full(cap, GUARD, np.uint32), off) for _ in range(2 + n_payload)]
            self.summary = (cap, self.sums[0].ptr, self.sums[1].ptr, [b.ptr for b in self.sums[2:]])

    def call(self, key_bits, init, want_rc=False, entry="chain"):
        if entry == "prev":
            args = [{k: v for k, v in a.items() if k not in ("row", "rule", "delta", "n_records", "span")} for a in self.args]
            return self.be.trace_prev_access(args, key_bits, self.np, init=init, summary=self.summary, want_rc=want_rc)
        return self.be.trace_access_chain(self.args, key_bits, self.np, init=init, summary=self.summary, want_rc=want_rc)

    def outputs(self):
        """every output word of the call, in a fixed order"""
        words = []
        for prev, ordinal in self.out:
            words += [b.read() for b in (prev or []) if b] + ([ordinal.read()] if ordinal else [])
        return words + [b.read() for b in self.sums or []]

    def check(self, want, n_keys):
        for s, (prev, ordinal) in enumerate(self.out):
            for c, b in enumerate(prev or []):
                if b:
                    got = b.read()
                    assert np.array_equal(got, want["prev"][s][c]), ("prev", s, c, np.flatnonzero(got != want["prev"][s][c])[:8])
            if ordinal:
                assert np.array_equal(ordinal.read(), want["ordinal"][s]), ("ordinal", s)
        assert n_keys == len(want["keys"])
        if self.summary:
            m = min(self.cap, len(want["keys"]))
            for name, b, exp in [("key", self.sums[0], want["keys"]), ("count", self.sums[1], want["counts"])] + [("last %d" % c, self.sums[2 + c], want["last"][c]) for c in range(self.np)]:
                got = b.read()
                assert np.array_equal(got[:m], exp[:m]), name
                assert (got[m:] == GUARD).all(), name + ": words behind the entries were written"
        assert all(b.untouched() for b in self.ins), "an input was written"


def run(be, nz, streams, key_bits, n_payload, init, cap=None, off=0, judge=M.model):
    want = judge(streams, key_bits, n_payload, init)
    assert want["bad"] is None
    d = Device(be, nz, streams, n_payload, cap, off)
    d.check(want, d.call(key_bits, init))
    return d, want


# ------------------------------------------------------------------------------------------------------------ 1. compatibility ----
def _both_entries(be, nz, streams, key_bits, n_payload, init, cap):
    words = []
    for entry in ("prev", "chain"):
        d = Device(be, nz, streams, n_payload, cap)
        n = d.call(key_bits, init, entry=entry)
        words.append((n, d.outputs()))
    assert words[0][0] == words[1][0]
    assert len(words[0][1]) == len(words[1][1]) and all(np.array_equal(a, b) for a, b in zip(*[w[1] for w in words]))
    assert not any((w == GUARD).all() for w in words[1][1] if len(w))
    return words[1]


@pytest.mark.parametrize("log_size", [2, 11])
def test_two_linear_streams_through_both_entries(be, nz, log_size):
    streams = PM.two_linear_streams(np.random.default_rng(2020), log_size)
    n, words = _both_entries(be, nz, streams, [8, 5], 1, [P - 3], cap=(1 << log_size) + 2)
    assert n == len(PM.model(streams, [8, 5], 1, [P - 3])["keys"])


def test_mixed_streams_through_both_entries(be, nz):
    """epochs, flags, NULL payload columns, outputs not wanted and bit-reversed streams of 2^1 .. 2^9 rows"""
    rng = np.random.default_rng(31)
    streams = [M.column_stream(rng, [8, 5], 5, 3, rng.integers(0, 1 << 7, 32), null_payload=(2,), epoch=0, linear=True, prev_wanted=None, want_ord=False)]
    for log in range(1, 10):
        streams.append(M.column_stream(rng, [8, 5], log, 3, rng.integers(0, 1 << 7, 1 << log), flags=bool(log % 3), null_payload=(log % 3,), epoch=1 + log % 2,
                                       prev_wanted=[True, log % 4 != 0, True], want_ord=log % 5 != 0))
    n, words = _both_entries(be, nz, streams, [8, 5], 3, [5, 6, 7], cap=200)
    want = M.model(streams, [8, 5], 3, [5, 6, 7])
    assert n == len(want["keys"])


# ------------------------------------------------------------------------- 2. chains across every boundary of the scan ----------
def _one_key(rng, n, given_at=None, delta=1, first_lane=0, other_keys=0):
    """a linear stream whose rows first_lane .. first_lane + n - 1 access key 77 by ADD (the rows before access smaller keys, `other_keys`
    rows behind a larger one, so that the run starts at sorted index first_lane), beside one GIVEN column; given_at: the one access of
    them that belongs to a second stream and is GIVEN in the chained column (an ADD column in one stream, GIVEN in another)"""
    log = max(1, int(first_lane + n + other_keys - 1).bit_length())
    size = 1 << log
    keys, flag = np.full(size, 77, np.uint64), np.zeros(size, np.uint32)
    keys[:first_lane] = np.arange(first_lane)
    keys[first_lane + n:first_lane + n + other_keys] = 100
    flag[:first_lane + n + other_keys] = 1
    a = M.column_stream(rng, [13], log, 2, keys, rule=[ADD, GIVEN], delta=[delta, 0], flags=flag, linear=True)
    if given_at is None:
        return [a]
    a["flag"][first_lane + given_at] = 0
    g = M.block_stream(rng, [13], [first_lane + given_at], 1, 2, [77])
    return [a, g]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 2049, 3000])
def test_one_key_chained_by_add(be, nz, n):
    """at 2049 and 3000 a whole block of 1024 sorted elements is pure ADD; then one GIVEN at the first, the middle and the last access"""
    rng = np.random.default_rng(n)
    d, want = run(be, nz, _one_key(rng, n), [13], 2, [0, 9], cap=1)
    assert want["last"][0][0] == n and np.array_equal(want["prev"][0][0][:n], np.arange(n))
    for at in sorted({0, n // 2, n - 1}):
        d, want = run(be, nz, _one_key(rng, n, given_at=at), [13], 2, [0, 9], cap=1)
        assert want["last"][0][0] == (int(want["left"][1][0][0]) + n - 1 - at) & 0xFFFFFFFF


@pytest.mark.parametrize("delta", [0, 1, 0xFFFFFFFF])
def test_deltas_and_a_nonzero_init(be, nz, delta):
    rng = np.random.default_rng(5)
    d, want = run(be, nz, _one_key(rng, 1500, delta=delta), [13], 2, [P - 1, 3], cap=1)
    assert want["last"][0][0] == (P - 1 + 1500 * delta) & 0xFFFFFFFF


@pytest.mark.parametrize("lane", [0, 1, 2, 3])
def test_runs_that_start_at_each_quad_lane_and_meet_at_a_block_edge(be, nz, lane):
    """the run of key 77 starts at sorted index `lane` and ends exactly at the edge of the first block of 1024: the run of key 100 begins
    the second one"""
    rng = np.random.default_rng(lane)
    streams = _one_key(rng, 1024 - lane, first_lane=lane, other_keys=1030)
    d, want = run(be, nz, streams, [13], 2, [7, 0], cap=8)
    assert want["keys"].tolist()[-2:] == [77, 100] and want["counts"].tolist()[-2:] == [1024 - lane, 1030]


def test_two_add_columns_beside_a_given_one_and_rules_that_differ_by_stream(be, nz):
    rng = np.random.default_rng(8)
    keys = lambda n: rng.integers(0, 40, n)
    streams = [M.column_stream(rng, [8, 5], 11, 3, keys(2048), rule=[ADD, GIVEN, ADD], delta=[1, 0, 0xFFFFFFF0], flags=True),
               M.column_stream(rng, [8, 5], 11, 3, keys(2048), rule=[GIVEN, GIVEN, ADD], delta=[0, 0, 3], null_payload=(1,)),
               M.column_stream(rng, [8, 5], 6, 3, keys(64), rule=[ADD, ADD, GIVEN], delta=None, epoch=1)]
    run(be, nz, streams, [8, 5], 3, [1, 2, 3], cap=40)


# ------------------------------------------------------------------------------------------------------------ 3. block streams ----
@pytest.mark.parametrize("span", [1, 4, 200, 256])
@pytest.mark.parametrize("n_records", [0, 1, 2, 5, 40])
def test_block_streams(be, nz, span, n_records):
    """records on consecutive rows and on the first and last row of the trace, at the row of an access of a column stream that lies
    earlier in `streams` and of one that lies later; 1, 2 or 8 block streams; overlapping buffers; bytes; record flags; column streams of
    2^2, 2^6 or 2^12 rows beside them"""
    v = [1, 4, 200, 256].index(span) * 5 + [0, 1, 2, 5, 40].index(n_records)
    rng = np.random.default_rng(300 + v)
    log, n_blocks, key_bits, npay = [2, 6, 12][v % 3], [1, 2, 8][(v // 3) % 3], [16, 16], 2
    if n_records > (1 << log):
        log = 6
    n = 1 << log
    base = 0xFFFF00                                                   # the buffers straddle a limb boundary of the key
    must = ([0] if n_records else []) + ([n - 1] if n_records > 1 else []) + ([n // 2, n // 2 + 1] if n_records > 3 else [])
    rows = np.array(sorted(set(must) | set([int(r) for r in rng.permutation(n) if r not in must][:n_records - len(set(must))])), np.uint32)
    assert len(rows) == n_records and (np.diff(rows) > 0).all()
    addr = lambda m: base + rng.integers(0, 3, m) * (span - span // 4)               # overlapping buffers
    col = lambda: M.column_stream(rng, key_bits, log, npay, base + rng.integers(0, 3 * span, n), flags=True, epoch=1)
    streams = [M.column_stream(rng, key_bits, 5, npay, base + np.arange(32), epoch=0, linear=True, prev_wanted=None, want_ord=False), col()]
    bytes_ok = span % 4 == 0
    streams.append(M.block_stream(rng, key_bits, rows, span, npay, addr(n_records), rule=[ADD, GIVEN | BYTES if bytes_ok else GIVEN], delta=[1, 0], flags=bool(v & 1), epoch=1))
    streams.append(col())
    for b in range(1, n_blocks):
        m = 1 + (b + v) % 3
        streams.append(M.block_stream(rng, key_bits, np.sort(rng.choice(n, m, replace=False)), span if b % 2 else 4, npay, addr(m), rule=[ADD, GIVEN], delta=[b, 0], epoch=1 + b // 6))
    run(be, nz, streams, key_bits, npay, [0, 0], cap=4 * span + 40, judge=M.model_by_sorting if log == 12 else M.model)


def test_bytes_and_words_of_the_same_values_give_the_same_outputs(be, nz):
    make = lambda rule: [M.column_stream(np.random.default_rng(1), [16, 16], 6, 2, 0x8000 + np.random.default_rng(2).integers(0, 300, 64), epoch=0),
                         M.block_stream(np.random.default_rng(3), [16, 16], [1, 2, 9, 63], 200, 2, [0x8000, 0x8000, 0x8040, 0x8000], rule=[ADD, rule], epoch=0)]
    a, b = make(GIVEN | BYTES), make(GIVEN)
    b[1]["payload"][1] = a[1]["payload"][1].copy()                    # the same values, one word each
    assert np.array_equal(a[1]["payload"][1], b[1]["payload"][1]) and a[1]["payload"][1].max() < 256
    da, want = run(be, nz, a, [16, 16], 2, [3, 4], cap=400)
    db, _ = run(be, nz, b, [16, 16], 2, [3, 4], cap=400)
    assert all(np.array_equal(x, y) for x, y in zip(da.outputs(), db.outputs()))


# ------------------------------------------------------------------------------------- 7. the RAM of a keccak guest, and 4. 6. ----
KEY_BITS = [16, 16]


@pytest.fixture(scope="module")
def ram():
    """a consistent history: what a record leaves is keccak-f[1600] of what it found (found by running the walk until it is stable:
    each pass settles at least the earliest record not yet settled)"""
    out = np.zeros((5, 200), np.uint32)
    for _ in range(8):
        streams, rows, addresses = M.keccak_ram_history(np.random.default_rng(64), 6, out)
        want = M.model(streams, KEY_BITS, 2, [0, 0])
        found = want["prev"][5][1].reshape(5, 200).astype(np.uint8)
        states = np.ascontiguousarray(found).view("<u8").reshape(5, 25)
        new = MM.keccak_f(states).view(np.uint8).reshape(5, 200).astype(np.uint32)
        if np.array_equal(new, out):
            break
        out = new
    else:
        raise AssertionError("the history did not settle")
    assert want["bad"] is None
    return streams, rows, addresses, states, want


def _keccak_on_device(be, nz, states):
    """keccak-f of the states by two nx_trace_keccak_round calls (16 rounds, then 8) -> the buffer the second one wrote as d_states_out"""
    from test_gpu_keccak_round import _states_on_device
    import keccak_round_model as R
    n = len(states)
    d_in, d_mid, d_fin = (_states_on_device(be, nz, x) for x in (states, np.zeros((n, 25), np.uint64), np.zeros((n, 25), np.uint64)))
    log_a, log_b = int(n * 16 - 1).bit_length(), int(n * 8 - 1).bit_length()
    be.trace_keccak_round(d_in.ptr.value, n, 0, 4, log_a, list(nz.DeviceColumns(be, R.MAIN_COLS, log_a).col_ptrs()), None, d_mid.ptr.value)
    be.trace_keccak_round(d_mid.ptr.value, n, 16, 3, log_b, list(nz.DeviceColumns(be, R.MAIN_COLS, log_b).col_ptrs()), None, d_fin.ptr.value)
    return d_in, d_fin


def test_the_ram_of_a_keccak_guest_end_to_end_on_the_device(be, nz, ram):
    streams, rows, addresses, states, want = ram
    assert (np.diff(rows[:3]) == 1).all() and addresses[0] == addresses[2] and addresses[3] - addresses[0] == 192           # A three times in a row; B overlaps it by 8
    d_in, d_fin = _keccak_on_device(be, nz, states)
    d = Device(be, nz, streams, 2, cap=1024, payload_ptrs={(5, 1): d_fin.ptr.value})
    n_keys = d.call(KEY_BITS, [0, 0])
    d.check(want, n_keys)                                                                     # Ram*TsPrev / ValPrev, the records' outputs, the summary
    assert np.array_equal(d_fin.to_cpu().reshape(-1)[:250].view(np.uint8).astype(np.uint32), streams[5]["payload"][1])       # what the round calls left is what the walk says
    ts_prev, val_prev = d.out[5][0]
    assert np.array_equal(val_prev.read().astype(np.uint8).view("<u8").reshape(5, 25), states)      # the records found their input states
    # the previous timestamps, as they lie, are the d_timestamps of the memory-check component
    assert ts_prev.ptr % 16 == 0
    main = nz.DeviceColumns(be, MM.MAIN_COLS, 3).upload(np.full((MM.MAIN_COLS, 8), GUARD, np.uint32))
    d_addr = Buf(be, nz, addresses)
    be.trace_keccak_memory_check(d_in.ptr.value, d_addr.ptr, ts_prev.ptr, 5, 3, list(main.col_ptrs()), None, None)
    model_main = MM.fill(states, addresses, want["prev"][5][0].reshape(5, 200), 3)["main"]
    assert np.array_equal(main.to_cpu(), model_main)
    # memory consistency in Python integers: what the accesses consume = the image + what the accesses leave - the final state
    consumed, produced = {}, {}
    bump = lambda bag, t: bag.__setitem__(t, bag.get(t, 0) + 1)
    outs = d.outputs()
    got_prev = {(s, c): b.read() for s, (prev, _) in enumerate(d.out) for c, b in enumerate(prev or []) if b}
    for s, st in enumerate(streams):
        for e in range(M.n_elems(st)):
            unit = e // st["span"] if M.is_block(st) else e
            if st.get("flag") is not None and st["flag"][unit] == 0:
                continue
            key = int(want["key"][s][e])
            left = (int(want["left"][s][0][e]), int(want["left"][s][1][e]))
            if s == 0:
                bump(consumed, (key, 0, 0))                                                    # the image writes over the untouched state
            else:
                bump(consumed, (key, int(got_prev[(s, 0)][e]), int(got_prev[(s, 1)][e])))
            if s == 5:
                left = ((int(got_prev[(s, 0)][e]) + 1) & 0xFFFFFFFF, left[1])                  # the record's next timestamp from the device's previous one
            bump(produced, (key, left[0], left[1]))
    m = n_keys
    assert m <= d.cap
    for k, ts, val in zip(d.sums[0].read()[:m].tolist(), d.sums[2].read()[:m].tolist(), d.sums[3].read()[:m].tolist()):
        bump(consumed, (k, ts, val))
        bump(produced, (k, 0, 0))
    assert consumed == produced and len(outs)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_placement(be, nz, ram, off):
    """every buffer at word offset 1, 2 and 3 inside its slab of guard words; the byte-packed payload stays 4-byte aligned"""
    streams, rows, addresses, states, want = ram
    d = Device(be, nz, streams, 2, cap=1024, off=off)
    assert all(a["key"][0] % 16 == 4 * off for a in d.args) and d.args[5]["payload"][1] % 4 == 0
    d.check(want, d.call(KEY_BITS, [0, 0]))


def test_same_words_on_two_runs_and_the_memory_bound(be, nz, ram):
    streams, rows, addresses, states, want = ram
    elems = sum(M.n_elems(st) for st in streams)
    d = Device(be, nz, streams, 2, cap=1024)
    be.sync()
    runs = []
    for _ in range(2):
        before = be.memory(reset_peak=True)
        d.call(KEY_BITS, [0, 0])
        live, peak = be.memory()
        assert live == before[0]                                                              # every temporary went back
        assert before[0] < peak <= before[0] + 18 * elems + 1024 * len(streams) + 65536     # the bound of the header
        runs.append(d.outputs())
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------------------------ 5. refusals ----
def _small(rng):
    return [M.column_stream(rng, [8, 5], 6, 2, rng.integers(0, 300, 64), rule=[ADD, GIVEN], flags=True),
            M.block_stream(rng, [8, 5], [1, 5, 9, 20, 63], 8, 2, rng.integers(0, 300, 5), rule=[ADD, GIVEN | BYTES], flags=np.ones(5, np.uint32)),
            M.block_stream(rng, [8, 5], [0, 7, 8], 4, 2, rng.integers(0, 300, 3), rule=[ADD, GIVEN])]


def test_refusals_through_a_live_context(be, nz):
    cases = []
    s = _small(np.random.default_rng(1)); s[1]["key"][0][3] = 256; s[2]["key"][1][0] = 32
    cases.append((s, "stream 1 record 3: key entry 0 holds 256, outside its 8 bits"))
    s = _small(np.random.default_rng(2)); s[1]["key"][0][2], s[1]["key"][1][2] = 250, 31
    cases.append((s, "stream 1 record 2 sub-access 6: key 8186 + 6 is outside the 13 key bits"))
    s = _small(np.random.default_rng(3)); s[2]["row"] = np.array([7, 7, 9], np.uint32)
    cases.append((s, "stream 2 record 1: d_row of 7 is not above its predecessor's 7"))
    s = _small(np.random.default_rng(4)); s[1]["row"] = np.array([1, 9, 5, 4, 30], np.uint32); s[2]["row"] = np.array([3, 2, 1], np.uint32)
    cases.append((s, "stream 1 record 2: d_row of 5 is not above its predecessor's 9"))
    s = _small(np.random.default_rng(5)); s[0]["key"][1][40], s[0]["flag"][40] = 32, 1; s[1]["row"] = np.array([5, 4, 3, 2, 1], np.uint32)
    cases.append((s, "stream 0 row position 40: key entry 1 holds 32, outside its 5 bits"))
    for streams, text in cases:
        want = M.model(streams, [8, 5], 2)
        assert want["bad"] is not None and want["bad"] == M.model_by_sorting(streams, [8, 5], 2)["bad"]
        d = Device(be, nz, streams, 2, cap=64)
        n, rc = d.call([8, 5], [0, 0], want_rc=True)
        msg = be.L.nx_last_error(be.ctx).decode()
        assert (n, rc) == (None, NX_ERR_PROTOCOL) and msg.startswith("nx_trace_access_chain: ") and text in msg, (msg, text)
        assert all(b.untouched() for b in d.ins)
        before = be.memory()
        run(be, nz, _small(np.random.default_rng(9)), [8, 5], 2, [0, 0], cap=64)              # the context then runs a good call
        assert be.memory()[0] == before[0]
    # an entry out of its bits on a record that does not access is no fault
    s = _small(np.random.default_rng(6)); s[1]["key"][0][3] = 999; s[1]["flag"][3] = 0
    run(be, nz, s, [8, 5], 2, [0, 0], cap=64)


# ----------------------------------------------------------------------------------------------------- 8. one whole statement ----
class _OnDevice(np.ndarray):
    """host words that also lie on the device (device: something with .ptr.value); side: the words the load/store stand-in is built from"""
    device = None
    side = None


def test_the_closed_keccak_statement_with_timestamps_from_the_chain(be, nz, monkeypatch):
    """The statement of tests/test_gpu_keccak_memcheck.py at its shape (3 instances), with d_timestamps being the buffer
    nx_trace_access_chain wrote for a history of stores and three records: two on one buffer, the third overlapping it by 8 bytes.
    mem_side stays the host-filled stand-in for the load/store chip, built from the WALK's timestamps.  Control: the second record
    moved before a store it depended on — the device's timestamps change, the stand-in's do not, and the sums no longer cancel."""
    import test_gpu_keccak_memcheck as KM
    from keccak_memcheck_air import COMPONENTS, MAIN_AT, N_INST, RELATIONS, TREE_LOGS, statement_inputs, total
    states, _, _ = statement_inputs()
    addresses = np.array([0xFFFE, 0xFFFE, 0xFFFE + 192], np.uint32)                            # a limb carry inside every buffer

    def history(rows):
        rng = np.random.default_rng(90)
        store_addr = 0xFFFE - 8 + rng.integers(0, 420, 16)
        store_addr[7] = 0xFFFE + 100                                                          # a store at row 7 into the first buffer
        st = M.column_stream(rng, KEY_BITS, 4, 1, store_addr[PM.rows_of_positions(4, False)].astype(np.uint64), epoch=1)
        st["payload"][0] = (np.arange(16, dtype=np.uint32) + 1)[PM.rows_of_positions(4, False)]
        return [st, M.block_stream(rng, KEY_BITS, rows, 200, 1, addresses.astype(np.uint64), rule=[ADD], delta=[1], epoch=1, want_ord=False)]

    def timestamps(rows):
        streams = history(rows)
        want = M.model(streams, KEY_BITS, 1, [0])
        d = Device(be, nz, streams, 1)
        d.check(want, d.call(KEY_BITS, [0]))
        ts = want["prev"][1][0].reshape(N_INST, 200).view(_OnDevice)
        ts.device = d.out[1][0][0].dev                                                        # the slab the call wrote (offset 0)
        return ts

    good, moved = timestamps([3, 9, 12]), timestamps([3, 5, 12])
    assert good[1, 100] == 8 and moved[1, 100] == 1 and not np.array_equal(good, moved)      # the store of row 7 (timestamp 8) now comes after the record
    words_on_device, host_statement = KM._words_on_device, KM.host_statement
    monkeypatch.setattr(KM, "_words_on_device", lambda be_, nz_, w: w.device if isinstance(w, _OnDevice) else words_on_device(be_, nz_, w))

    def statement_with_side(st, addr, ts):
        pre, main, final = host_statement(st, addr, np.asarray(ts))
        if getattr(ts, "side", None) is not None:
            main[MAIN_AT["mem_side"]:] = host_statement(st, addr, np.asarray(ts.side))[1][MAIN_AT["mem_side"]:]
        return pre, main, final
    monkeypatch.setattr(KM, "host_statement", statement_with_side)

    claimed, (s, cfg, comps, roots, drawn, host_pre, host_main) = KM._session(be, nz, (states, addresses, good))
    assert total(claimed) == [0, 0, 0, 0] and all(np.asarray(claimed[name]).any() for name in COMPONENTS)
    report = s.check(comps)
    assert report.ok, report
    words = s.prove(comps)
    v = nz.VerifierSession(cfg)
    v.mix_u64(5)
    v.commit(roots[0], TREE_LOGS[0])
    v.commit(roots[1], TREE_LOGS[1])
    assert np.array_equal(v.draw_felts(2 * len(RELATIONS)), drawn)
    v.mix_felts(np.array([claimed[name] for name in COMPONENTS], np.uint32))
    v.commit(roots[2], TREE_LOGS[2])
    assert v.verify(comps, words) is None
    s.close()
    moved.side = np.asarray(good)
    off, (s2, *_rest) = KM._session(be, nz, (states, addresses, moved))
    s2.close()
    assert total(off) != [0, 0, 0, 0]
