"""nx_trace_prev_access on the device against the sequential dictionary model of tests/prev_access_model.py.  Every comparison is an
equality of words.
1. key shapes [5] (one radix pass), [8, 5] (two), [8, 8, 8, 8] (four; five with flags) and [31]; 2^1, 2^2, 2^6, 2^11 and 2^14 rows (two
   rows, the tail of a tile, several blocks, the wrap between the halves of the circle domain); one, three and four streams; with and
   without flags, ordinal and summary; 1, 5, 8 and 16 payload columns, some payload and output entries NULL; 2^20 + 2 rows, where a block of
   the sort takes more than its minimum of tiles;
2. skew;  3. epochs and mixed sizes;  4. the summary;  5. a key entry out of its bits;  6. determinism and memory;
7. a register-file-shaped statement through a prover session: narrow seed columns, timestamps from nx_trace_program, previous-access
   columns and the final-state table from nx_trace_prev_access; the memory-check logup cancels, the statement is proved and verified."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import prev_access_model as M

pytestmark = pytest.mark.gpu
P = M.P
NX_OK, NX_ERR_ARG, NX_ERR_PROTOCOL = 0, -2, -4
GUARD = 0xDEADBEEF


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


def _split(keys, key_bits):
    out, shift = [], 0
    for b in key_bits:
        out.append(((np.asarray(keys, np.uint64) >> np.uint64(shift)) & np.uint64((1 << b) - 1)).astype(np.uint32))
        shift += b
    return out


def make_stream(rng, key_bits, log_size, n_payload, keys=None, flags=False, null_payload=(), prev_wanted=None, want_ord=True, epoch=0, linear=False, zero_payload=()):
    """a stream of host columns; keys default to draws from a pool a quarter the size of the stream, so that keys repeat in wide key
    spaces too"""
    n, total = 1 << log_size, sum(key_bits)
    if keys is None:
        pool = rng.integers(0, min(1 << total, P), size=max(1, n // 4), dtype=np.uint64)
        keys = pool[rng.integers(0, len(pool), size=n)]
    pay = [None if c in null_payload else (np.zeros(n, np.uint32) if c in zero_payload else rng.integers(0, P, size=n, dtype=np.uint32)) for c in range(n_payload)]
    return {"key": _split(keys, key_bits), "flag": (rng.integers(0, 3, size=n, dtype=np.uint32) * rng.integers(1, 9, size=n, dtype=np.uint32)) if flags else None,
            "payload": pay, "log_size": log_size, "epoch": epoch, "linear": linear,
            "prev_wanted": [True] * n_payload if prev_wanted is None else prev_wanted, "want_ord": want_ord}


class Device:
    """the streams on the device: inputs uploaded, outputs filled with a guard word"""

    def __init__(self, be, nz, streams, n_payload, cap=None, guard=4):
        self.be, self.nz, self.streams, self.np, self.keep, self.args, self.out = be, nz, streams, n_payload, [], [], []
        for st in streams:
            log, n = st["log_size"], 1 << st["log_size"]
            kc = self.cols(np.stack(st["key"]), log)
            flag = self.cols(st["flag"][None, :], log)[0] if st["flag"] is not None else None
            pay = [self.cols(p[None, :], log)[0] if p is not None else None for p in st["payload"]]
            prev = None
            if st["prev_wanted"] is not None:
                prev = [self.cols(np.full((1, n), GUARD, np.uint32), log)[0] if w else None for w in st["prev_wanted"]]
            ordinal = self.cols(np.full((1, n), GUARD, np.uint32), log)[0] if st["want_ord"] else None
            self.args.append({"key": kc, "flag": flag, "payload": pay, "prev": prev, "ordinal": ordinal, "log_size": log, "epoch": st["epoch"], "linear": st["linear"]})
            self.out.append((prev, ordinal))
        self.cap, self.summary = cap, None
        if cap is not None:
            self.sum_log = max(1, int(cap + guard - 1).bit_length())
            arrs = self.cols(np.full((2 + n_payload, 1 << self.sum_log), GUARD, np.uint32), self.sum_log)
            self.summary = (cap, arrs[0], arrs[1], arrs[2:])

    def cols(self, arr2d, log):
        d = self.nz.DeviceColumns(self.be, arr2d.shape[0], log).upload(arr2d)
        self.keep.append(d)
        return [d.ptr.value + i * (4 << log) for i in range(arr2d.shape[0])]

    def read(self, ptr, log):
        return self.nz.DeviceColumns.view(self.be, ptr, 1, log).to_cpu().reshape(-1)

    def call(self, key_bits, init, want_rc=False):
        return self.be.trace_prev_access(self.args, key_bits, self.np, init=init, summary=self.summary, want_rc=want_rc)

    def outputs(self):
        """every output word of the call, in a fixed order"""
        words = []
        for st, (prev, ordinal) in zip(self.streams, self.out):
            words += [self.read(p, st["log_size"]) for p in (prev or []) if p] + ([self.read(ordinal, st["log_size"])] if ordinal else [])
        if self.summary:
            words += [self.read(p, self.sum_log) for p in [self.summary[1], self.summary[2]] + list(self.summary[3])]
        return words

    def check(self, want, n_keys):
        for s, (st, (prev, ordinal)) in enumerate(zip(self.streams, self.out)):
            for c, p in enumerate(prev or []):
                if p:
                    assert np.array_equal(self.read(p, st["log_size"]), want["prev"][s][c]), ("prev", s, c)
            if ordinal:
                assert np.array_equal(self.read(ordinal, st["log_size"]), want["ordinal"][s]), ("ordinal", s)
        assert n_keys == len(want["keys"])
        if self.summary:
            m = min(self.cap, len(want["keys"]))
            for name, ptr, exp in [("key", self.summary[1], want["keys"]), ("count", self.summary[2], want["counts"])] + \
                                  [("last %d" % c, self.summary[3][c], want["last"][c]) for c in range(self.np)]:
                got = self.read(ptr, self.sum_log)
                assert np.array_equal(got[:m], exp[:m]), name
                assert (got[m:] == GUARD).all(), name + ": words behind the entries were written"


def run(be, nz, streams, key_bits, n_payload, init, cap=None):
    want = M.model(streams, key_bits, n_payload, init)
    assert want["bad"] is None
    d = Device(be, nz, streams, n_payload, cap)
    d.check(want, d.call(key_bits, init))
    return d, want


KEYINGS = [[5], [8, 5], [8, 8, 8, 8], [31]]
LOGS = [1, 2, 6, 11, 14]


@pytest.mark.parametrize("key_bits", KEYINGS, ids=lambda b: "bits" + "_".join(map(str, b)))
@pytest.mark.parametrize("log_size", LOGS)
def test_exact_against_the_model(be, nz, key_bits, log_size):
    """the other choices rotate with the case, so that every stream count, payload width and output choice meets small and large sizes
    and short and long keys"""
    v = KEYINGS.index(key_bits) * len(LOGS) + LOGS.index(log_size)
    rng = np.random.default_rng(1000 + v)
    n_streams, n_payload = [1, 3, 4][v % 3], [1, 5, 8, 16][(v // 3 + v) % 4]
    flags, want_ord, with_summary, nulls = bool(v & 1), bool((v >> 1) & 1) or v % 5 == 0, bool((v >> 2) & 1), v % 3 != 1
    streams = []
    for s in range(n_streams):
        null_payload = {(s + 1) % n_payload, (s + 4) % n_payload} if nulls and n_payload > 1 else set()
        prev_wanted = [not (nulls and (c + s) % 3 == 2) for c in range(n_payload)]
        streams.append(make_stream(rng, key_bits, log_size, n_payload, flags=flags and s != 1, null_payload=null_payload, prev_wanted=prev_wanted,
                                   want_ord=want_ord or s == 0))
    init = rng.integers(0, P, size=n_payload, dtype=np.uint32)
    run(be, nz, streams, key_bits, n_payload, init, cap=(n_streams << log_size) if with_summary else None)


def test_a_sort_block_of_more_than_the_minimum_tiles(be, nz):
    """2^20 + 2 elements in one epoch: more than 1024 blocks of four tiles, so a block of each of the two sort passes takes five (the path
    the host emulation reaches with a block cap of 2).  Judged by M.model_by_sorting, which tests/test_prev_access_cpu.py holds to the
    sequential model."""
    streams = M.two_linear_streams(np.random.default_rng(2020), 20)
    key_bits, init = [8, 5], np.array([P - 3], np.uint32)
    want = M.model_by_sorting(streams, key_bits, 1, init)
    assert want["bad"] is None and len(want["keys"]) == 1 << 13
    d = Device(be, nz, streams, 1, cap=1 << 13)
    d.check(want, d.call(key_bits, init))


@pytest.mark.parametrize("key_bits", [[8, 5], [8, 8, 8, 8]], ids=["bits8_5", "bits8_8_8_8"])
def test_skew(be, nz, key_bits):
    rng = np.random.default_rng(7)
    log, n, npay = 11, 1 << 11, 5
    init = np.array([P - 1, 7, 0, P - 2, 1], np.uint32)
    one = [make_stream(rng, key_bits, log, npay, keys=np.full(n, 0x1A5A, np.uint64) & np.uint64((1 << sum(key_bits)) - 1)) for _ in range(3)]
    d, want = run(be, nz, one, key_bits, npay, init, cap=4)          # the chain is the whole trace
    assert len(want["keys"]) == 1 and want["counts"][0] == 3 * n
    distinct = [make_stream(rng, key_bits, log - 1, npay, keys=rng.permutation(n // 2).astype(np.uint64) * np.uint64(3) + np.uint64(s)) for s in range(3)]
    d, want = run(be, nz, distinct, key_bits, npay, init, cap=3 * n // 2)     # every access takes init
    assert len(want["keys"]) == 3 * n // 2
    for s in range(3):
        for c in range(npay):
            assert (want["prev"][s][c] == init[c]).all()
    half = [make_stream(rng, key_bits, log, npay, keys=(rng.integers(0, 8, size=n, dtype=np.uint64) == 0) * rng.integers(0, 1 << 13, size=n, dtype=np.uint64),
                        zero_payload=(1, 3), flags=bool(s & 1)) for s in range(4)]
    run(be, nz, half, key_bits, npay, init, cap=1 << 13)


def test_epochs_and_mixed_sizes(be, nz):
    """RAM-shaped: a linear image of 2^7 addresses in epoch 0 (no outputs), four byte streams of 2^10 rows in epoch 1, the address as
    four byte limbs.  Natural row r < 128 touches imaged address 2 r with all four streams, the later rows touch odd addresses, which
    were never imaged."""
    rng = np.random.default_rng(11)
    key_bits, npay = [8, 8, 8, 8], 5
    init = np.array([0, P - 1, 3, 0, 9], np.uint32)
    image = make_stream(rng, key_bits, 7, npay, keys=0x10000 + 2 * np.arange(128, dtype=np.uint64), epoch=0, linear=True, want_ord=False)
    image["prev_wanted"] = None
    rows = np.arange(1024, dtype=np.uint64)
    addr = np.where(rows < 128, 0x10000 + 2 * rows, 0x10001 + 2 * (rows % 300))
    streams = [image] + [make_stream(rng, key_bits, 10, npay, keys=M.to_storage(addr, 10), epoch=1) for _ in range(4)]
    d, want = run(be, nz, streams, key_bits, npay, init, cap=1024)
    nat = M.rows_of_positions(10, False)                            # natural row of every storage position
    for c in range(npay):
        first = d.read(d.out[1][0][c], 10)
        assert np.array_equal(first[nat < 128], image["payload"][c][nat[nat < 128]])      # the first touch of an imaged address reads the image
        assert (first[(nat >= 128) & (nat < 428)] == init[c]).all()                     # never imaged: init
        for s in range(2, 5):                                                          # inside a row: the array order of the streams
            assert np.array_equal(d.read(d.out[s][0][c], 10), streams[s - 1]["payload"][c])
    assert np.array_equal(d.read(d.out[4][1], 10)[nat < 128], np.full(128, 4, np.uint32))
    # a third size in epoch 1 and a later epoch, flags on some
    more = streams + [make_stream(rng, key_bits, 6, npay, keys=M.to_storage(0x10000 + np.arange(64, dtype=np.uint64), 6), epoch=1, flags=True),
                      make_stream(rng, key_bits, 0, npay, keys=np.array([0x10002], np.uint64), epoch=1, linear=True),
                      make_stream(rng, key_bits, 3, npay, keys=M.to_storage(0x10000 + np.arange(8, dtype=np.uint64), 3), epoch=7)]
    run(be, nz, more, key_bits, npay, init, cap=1024)


def test_summary_shorter_than_the_keys(be, nz):
    rng = np.random.default_rng(13)
    key_bits, npay = [8, 5], 2
    streams = [make_stream(rng, key_bits, 9, npay, flags=bool(s)) for s in range(3)]
    want = M.model(streams, key_bits, npay, None)
    n_keys = len(want["keys"])
    assert n_keys > 40 and (np.diff(want["keys"].astype(np.int64)) > 0).all()
    for cap in (n_keys, 37, 1, 0):
        d = Device(be, nz, streams, npay, cap)
        d.check(want, d.call(key_bits, None))                       # exactly min(cap, n_keys) entries, the guard words behind them untouched, the true n_keys


def test_key_entry_out_of_its_bits(be, nz):
    rng = np.random.default_rng(17)
    key_bits, npay, log = [8, 5], 2, 11
    streams = [make_stream(rng, key_bits, log, npay, flags=s != 0) for s in range(3)]
    streams[1]["key"][0][1234] = 256
    streams[1]["flag"][1234] = 0
    streams[2]["key"][1][77] = P - 1
    streams[2]["flag"][77] = 0
    run(be, nz, streams, key_bits, npay, None)                        # on rows that do not access: ignored
    streams[1]["flag"][1234] = 2
    streams[2]["flag"][77] = 1
    streams[2]["key"][0][5] = 300
    streams[2]["flag"][5] = 1
    assert M.model(streams, key_bits, npay)["bad"] == (1, 1234)
    d = Device(be, nz, streams, npay)
    n_keys, rc = d.call(key_bits, None, want_rc=True)
    assert rc == NX_ERR_PROTOCOL and n_keys is None
    msg = be.L.nx_last_error(be.ctx).decode()
    assert "nx_trace_prev_access: stream 1 row position 1234: key entry 0 holds 256, outside its 8 bits" in msg, msg
    streams[1]["flag"][1234] = 0                                      # the smallest is now in stream 2, second entry
    streams[2]["flag"][5] = 0
    d = Device(be, nz, streams, npay)
    assert d.call(key_bits, None, want_rc=True) == (None, NX_ERR_PROTOCOL)
    assert "stream 2 row position 77: key entry 1 holds %d, outside its 5 bits" % (P - 1) in be.L.nx_last_error(be.ctx).decode()
    with pytest.raises(nz.NexusHipError):
        d.call(key_bits, None)
    streams[2]["flag"][77] = 0                                        # the context works afterwards
    run(be, nz, streams, key_bits, npay, None)


def test_same_words_on_two_runs_and_nothing_kept(be, nz):
    rng = np.random.default_rng(19)
    key_bits, npay, log = [8, 8, 8, 8], 5, 12
    streams = [make_stream(rng, key_bits, log, npay, flags=s == 2) for s in range(4)]
    init = rng.integers(0, P, size=npay, dtype=np.uint32)
    a, b = Device(be, nz, streams, npay, cap=1 << 14), Device(be, nz, streams, npay, cap=1 << 14)
    be.sync()
    live0, _ = be.memory(reset_peak=True)
    na = a.call(key_bits, init)
    live1, peak = be.memory()
    nb = b.call(key_bits, init)
    assert live1 == live0 and be.memory()[0] == live0           # every temporary went back to the allocator
    rows = 4 << log
    assert 16 * rows <= peak - live0 <= 18 * rows + 1024 * len(streams) + 65536      # the bound of include/nexus_hip.h
    assert na == nb
    for x, y in zip(a.outputs(), b.outputs()):
        assert np.array_equal(x, y)
    a.check(M.model(streams, key_bits, npay, init), na)


# ---------------------------------------------------------------- 7. the closed loop through a prover session ----------
# Component A, 2^8 rows, three register slots of 18 columns each: flag, address, 4 value limbs, 4 current-timestamp limbs, 4 previous
# timestamp limbs, 4 previous value limbs.  Component T, 32 rows: the register index (preprocessed, value i at position i) and the final
# timestamp and value limbs of every register.  Memory-check logup: + flag / (addr, ts_cur, val_cur) - flag / (addr, ts_prev, val_prev)
# per slot, + 1 / (reg, 0 .. 0) - 1 / (reg, final) per register: written - read + init - final = 0.
LOG_A, LOG_T, SLOT = 8, 5, 18
TREE_LOGS = [[LOG_T], [LOG_A] * (3 * SLOT) + [LOG_T] * 8, [LOG_A] * 24 + [LOG_T] * 8]


def _seed_columns():
    """per slot, in natural row order: flag, address, 4 value limbs as bytes; every register is touched, the last 16 rows are padding"""
    rng = np.random.default_rng(606)
    n = 1 << LOG_A
    slots = []
    for s in range(3):
        flag = (rng.random(n) < 0.8).astype(np.uint8)
        addr = rng.integers(0, 32, n).astype(np.uint8)
        if s == 0:
            flag[:32], addr[:32] = 1, np.arange(32)
        flag[n - 16:] = 0
        slots.append([flag, addr] + [rng.integers(0, 256, n).astype(np.uint8) for _ in range(4)])
    return slots


def _limbs(x):
    return [((np.asarray(x, np.uint32) >> (8 * j)) & 255).astype(np.uint32) for j in range(4)]


def _host_main_columns(slots):
    """every main column in storage order, computed on the host with the model: what a host without the device calls would upload"""
    n = 1 << LOG_A
    cols, streams = [], []
    for s, (flag, addr, *val) in enumerate(slots):
        ts = _limbs(3 * (np.arange(n) + 1) + s + 1)                 # 3 clk + slot, clk = row + 1
        nat = [flag, addr] + val + ts
        streams.append({"key": [M.to_storage(addr.astype(np.uint32), LOG_A)], "flag": M.to_storage(flag.astype(np.uint32), LOG_A),
                        "payload": [M.to_storage(np.asarray(c, np.uint32), LOG_A) for c in ts + val], "log_size": LOG_A})
        cols.append([M.to_storage(np.asarray(c, np.uint32), LOG_A) for c in nat])
    want = M.model(streams, [5], 8)
    main = []
    for s in range(3):
        main += cols[s] + want["prev"][s]                           # ts_prev limbs, then val_prev limbs
    assert want["keys"].tolist() == list(range(32))
    return main + want["last"], want


def _mem_programs(ap, z, alpha, shifts):
    pa = ap.ProgramBuilder()
    c = [pa.next_trace_mask(k)[0] for k in range(3 * SLOT)]
    rel = pa.relation(z, alpha, 9)
    for s in range(3):
        b = SLOT * s
        flag, addr, val, ts, tsp, valp = c[b], c[b + 1], c[b + 2:b + 6], c[b + 6:b + 10], c[b + 10:b + 14], c[b + 14:b + 18]
        pa.add_constraint(flag * (flag - 1))
        pa.add_to_relation(rel, flag, [addr] + ts + val)
        pa.add_to_relation(rel, -flag, [addr] + tsp + valp)
    pa.finalize_logup(3 * SLOT, shifts[0])
    pt = ap.ProgramBuilder()
    t = [pt.next_trace_mask(k)[0] for k in range(9)]                   # register index (preprocessed), final ts limbs, final value limbs
    rel = pt.relation(z, alpha, 9)
    pt.add_to_relation(rel, 1, [t[0]] + [0] * 8)
    pt.add_to_relation(rel, -1, t)
    pt.finalize_logup(9, shifts[1])
    return pa, pt


def _upload(be, ptr, host):
    host = np.ascontiguousarray(host, np.uint32)
    be._chk(be.L.nx_upload(be.ctx, C.c_void_p(ptr), host.ctypes.data_as(C.c_void_p), C.c_size_t(len(host))))


def _memcheck_session(be, nz, tamper):
    import nexus_zkvm_amd.air_program as ap
    cfg = nz.default_config(pow_bits=2)
    slots = _seed_columns()
    host_main, want = _host_main_columns(slots)
    regs = np.arange(1 << LOG_T, dtype=np.uint32)
    s = be.prover_session(cfg, LOG_A)
    s.mix_u64(3)
    roots = [s.commit([regs])]
    table = be.columns_from_host(regs)
    main = s.tree_begin(TREE_LOGS[1])
    # seeds: uploaded narrow, in natural row order
    arrs, kinds = nz._narrow_columns([c for sl in slots for c in sl])
    dst = (C.c_void_p * len(arrs))(*[main[SLOT * k + j] for k in range(3) for j in range(6)])
    be._chk(be.L.nx_upload_columns_narrow(be.ctx, *nz._host_columns(arrs, kinds), len(arrs), LOG_A, dst, 1))
    # current timestamps: 3 (row + 1) + slot from the natural row, as byte limbs
    tp = ap.ProgramBuilder()
    for k in range(3):
        ts = tp.row() * 3 + (4 + k)
        for j in range(4):
            tp.store(SLOT * k + 6 + j, tp.band(tp.shr(ts, 8 * j), 255))
    be.trace_program(tp.build_trace_program(), main[:3 * SLOT], LOG_A)
    # previous accesses, and the final state straight into the table component's columns
    skey, scount = be.columns(1, LOG_T), be.columns(1, LOG_T)
    streams = [{"key": [main[SLOT * k + 1]], "flag": main[SLOT * k], "payload": main[SLOT * k + 6:SLOT * k + 10] + main[SLOT * k + 2:SLOT * k + 6],
                "prev": main[SLOT * k + 10:SLOT * k + 18], "log_size": LOG_A} for k in range(3)]
    assert be.trace_prev_access(streams, [5], 8, summary=(32, skey.ptr.value, scount.ptr.value, main[3 * SLOT:])) == 32
    assert skey.to_cpu().reshape(-1).tolist() == list(range(32)) and np.array_equal(scount.to_cpu().reshape(-1), want["counts"])
    got = [nz.DeviceColumns.view(be, d, 1, lg).to_cpu().reshape(-1) for d, lg in zip(main, TREE_LOGS[1])]
    for k, (g, h) in enumerate(zip(got, host_main)):
        assert np.array_equal(g, h), "main column %d" % k
    if tamper:                                                          # one previous-timestamp word of an accessing row
        pos = int(np.flatnonzero(got[0])[5])
        col = got[10].copy()
        col[pos] = (int(col[pos]) + 1) % P
        _upload(be, main[10], col)
    kept = [be.clone_columns(nz.DeviceColumns.view(be, d, 1, lg)) for d, lg in zip(main, TREE_LOGS[1])]      # the commit turns columns into coefficients
    roots.append(s.tree_commit())
    z, alpha = s.draw_felt(), s.draw_felt()
    fracs = [p.build_logup() for p in _mem_programs(ap, z, alpha, [(0, 0, 0, 0)] * 2)]
    inter = s.tree_begin(TREE_LOGS[2])
    ins = [[k.ptr.value for k in kept[:3 * SLOT]], [table.ptr.value] + [k.ptr.value for k in kept[3 * SLOT:]]]
    claimed, shifts = [], []
    for frac, cols, out, log in zip(fracs, ins, [inter[:24], inter[24:]], [LOG_A, LOG_T]):
        assert 4 * frac.n_logup_cols == len(out)
        be.logup_program(frac, cols + [None] * len(out), log, out_ptrs=out)
        claimed.append(be.logup_finalize_last(out[-4:], log_size=log))
        n_inv = pow((1 << log) % P, P - 2, P)
        shifts.append([(int(x) * n_inv) % P for x in claimed[-1]])
    claimed = np.array(claimed, np.uint32)
    if tamper:
        s.close()
        return claimed, None
    s.mix_felts(claimed)
    roots.append(s.tree_commit())
    pa, pt = _mem_programs(ap, z, alpha, shifts)
    comps = [ap.Component(LOG_A, pa.build(), [(1, k) for k in range(3 * SLOT)] + [(2, k) for k in range(24)]),
             ap.Component(LOG_T, pt.build(), [(0, 0)] + [(1, 3 * SLOT + k) for k in range(8)] + [(2, 24 + k) for k in range(8)])]
    return claimed, (s, cfg, comps, roots, (z, alpha), host_main)


def test_a_memory_checked_statement_filled_on_the_device_is_proved_and_verified(be, nz):
    claimed, (s, cfg, comps, roots, (z, alpha), host_main) = _memcheck_session(be, nz, tamper=False)
    assert [int(sum(int(c[q]) for c in claimed) % P) for q in range(4)] == [0, 0, 0, 0]      # written - read + init - final = 0 (machine.rs:343)
    assert all(c.any() for c in claimed)
    report = s.check(comps)
    assert report.ok, report
    words = s.prove(comps)
    v = nz.VerifierSession(cfg)
    v.mix_u64(3)
    v.commit(roots[0], TREE_LOGS[0])
    v.commit(roots[1], TREE_LOGS[1])
    assert np.array_equal(v.draw_felt(), z) and np.array_equal(v.draw_felt(), alpha)
    v.mix_felts(claimed)
    v.commit(roots[2], TREE_LOGS[2])
    assert v.verify(comps, words) is None
    assert np.array_equal(v.digest(), s.digest())
    s.close()
    # the same main tree from a session fed the model's columns by the host: byte-equal root
    h = be.prover_session(cfg, LOG_A)
    h.mix_u64(3)
    assert np.array_equal(h.commit([np.arange(1 << LOG_T, dtype=np.uint32)]), roots[0])
    for d, col in zip(h.tree_begin(TREE_LOGS[1]), host_main):
        _upload(be, d, col)
    assert np.array_equal(h.tree_commit(), roots[1])
    h.close()
    # the control: one previous-timestamp word changed after the fill and the sums no longer cancel
    off, _ = _memcheck_session(be, nz, tamper=True)
    assert [int(sum(int(c[q]) for c in off) % P) for q in range(4)] != [0, 0, 0, 0]
