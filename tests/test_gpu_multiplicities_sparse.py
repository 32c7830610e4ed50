"""nx_logup_multiplicities_sparse on the device against the numpy model of tests/multiplicity_sparse_model.py (sorted valid keys,
searchsorted, exact Python-integer sums mod p = 2^31 - 1).  Every comparison is an equality.
1. exact against the model over key shapes, table sizes (up to the first one the LDS does not hold whole), valid-row patterns and
   mixed uses;  2. key extremes;  3. skew and 64-bit sums;  4. missing and out-of-range rows;  5. refusals;  6. memory and
   determinism;  7. agreement with nx_logup_multiplicities where both apply;  8. placement at word offsets 0..3 between guards;
9. a v2-shaped read/write-address statement (accesses + boundary) filled entirely on the device, proved and verified."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import multiplicity_sparse_model as M
import placement as PL

pytestmark = pytest.mark.gpu
P = M.P
NX_OK, NX_ERR_ARG, NX_ERR_PROTOCOL = 0, -2, -4
FILL = 0xDEADBEEF
MS_TILE_LOG = 12        # multiplicity_sparse.hip: MS_TILE = MS_THREADS * MS_QUADS * 4 = 4096 rows; a use of whole aligned tiles is read 16 bytes at a time


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


def _ptrs(d, n):
    return [d.ptr.value + k * (4 << d.log_size) for k in range(n)]


def run(be, uses, table, valid, key_bits, prefill=FILL):
    """Uploads, calls, reads back: (mult words, (n_missing, first_use, first_pos), rc)."""
    keep, dev_uses = [], []
    for cols, w in uses:
        d = be.columns_from_host(np.stack([np.asarray(c, np.uint32) for c in cols]))
        dw = be.columns_from_host(np.asarray(w, np.uint32)) if w is not None else None
        keep += [d, dw]
        dev_uses.append((_ptrs(d, len(cols)), dw.ptr.value if dw is not None else None, d.log_size))
    t = be.columns_from_host(np.stack([np.asarray(c, np.uint32) for c in table]))
    v = be.columns_from_host(np.asarray(valid, np.uint32)) if valid is not None else None
    out = be.columns_from_host(np.full(len(table[0]), prefill, np.uint32))
    res, rc = be.logup_multiplicities_sparse(dev_uses, _ptrs(t, len(table)), v.ptr.value if v is not None else None, t.log_size, key_bits, out.ptr.value, want_rc=True)
    return out.to_cpu().reshape(-1), res, rc


def check(be, uses, table, valid, key_bits):
    want, missing = M.multiplicities(uses, table, valid, key_bits)
    got, res, rc = run(be, uses, table, valid, key_bits)
    assert np.array_equal(got, want)
    if missing:
        assert rc == NX_ERR_PROTOCOL and res == (len(missing),) + missing[0]
    else:
        assert rc == NX_OK and res == (0, 0, 0)
    return got, missing


def make_table(rng, key_bits, log_table, mode, keys=None):
    """mode "all": every row valid (as far as the key space has keys), "half", "one", "none".  The rows that are no table rows hold
    garbage: copies of valid keys and values outside their bits.  -> (columns, valid column or None, the valid keys ascending)"""
    tb, n = sum(key_bits), 1 << log_table
    want = {"all": n, "half": (n + 1) // 2, "one": 1, "none": 0}[mode]
    want = min(want, 1 << tb)
    if keys is None:
        keys = set()
        while len(keys) < want:
            keys.update(rng.integers(0, 1 << tb, want - len(keys), dtype=np.uint64).tolist())
        keys = np.array(sorted(keys), np.uint64)
    want = len(keys)
    where = rng.permutation(n)
    table = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in key_bits]
    valid = np.zeros(n, np.uint32)
    for c, col in zip(table, M.split(rng.permutation(keys), key_bits)):
        c[where[:want]] = col
    valid[where[:want]] = rng.integers(1, 1 << 32, want, dtype=np.uint64).astype(np.uint32)
    if want:
        rest = where[want:][::2]
        src = where[rng.integers(0, want, len(rest))]
        for c in table:
            c[rest] = c[src]
    return table, (None if want == n else valid), keys


def make_use(rng, key_bits, keys, log, weights, stray=0.01):
    m, tb = 1 << log, sum(key_bits)
    pick = keys[rng.integers(0, len(keys), m)] if len(keys) else rng.integers(0, 1 << tb, m, dtype=np.uint64)
    pick = np.where(rng.random(m) < stray, rng.integers(0, 1 << tb, m, dtype=np.uint64), pick)
    w = rng.choice(np.array([0, 1, 2, P - 1, P - 2], np.uint32), m) if weights else None
    return (M.split(pick, key_bits), w)


# ---------------------------------------------------------------- 1. exact against the model ----------
def _table_logs(nz):
    L = nz.MULT_SPARSE_LDS_LOG_KEYS     # multiplicity_sparse.hip: log_stride = log_table > MS_LDS_LOG_KEYS ? ... : 0 — a larger table is searched in two levels
    assert L + 1 <= 13
    return [0, 1, 2, 6, 8, 10, L + 1]


USE_LOGS = (0, 1, 2, 6, 12, 16)


@pytest.mark.parametrize("which_table", range(7))
@pytest.mark.parametrize("key_bits", [[32], [16, 16], [8, 8, 8, 8], [20], [1]], ids=lambda b: "bits" + "_".join(map(str, b)))
def test_counts_equal_the_model(be, nz, key_bits, which_table):
    log_table = _table_logs(nz)[which_table]
    rng = np.random.default_rng([sum(key_bits), len(key_bits), log_table])
    for mode in ("all", "half", "one", "none"):
        table, valid, keys = make_table(rng, key_bits, log_table, mode)
        uses = [make_use(rng, key_bits, keys, log, weights) for weights in (False, True) for log in USE_LOGS]
        order = rng.permutation(len(uses))
        got, _ = check(be, [uses[i] for i in order], table, valid, key_bits)
        if valid is not None:
            assert not got[valid == 0].any()
        if mode == "none" and sum(key_bits) > 1:
            assert not got.any()


def test_no_use_at_all_gives_a_zero_column(be):
    rng = np.random.default_rng(5)
    table, valid, _ = make_table(rng, [16, 16], 6, "half")
    got, missing = check(be, [], table, valid, [16, 16])
    assert not got.any() and not missing


# ---------------------------------------------------------------- 2. key extremes ----------
@pytest.mark.parametrize("key_bits", [[32], [16, 16], [8, 8, 8, 8]], ids=lambda b: "bits" + "_".join(map(str, b)))
def test_key_extremes(be, key_bits):
    rng = np.random.default_rng(len(key_bits))
    top = 0xABCDEF00
    sets = {
        "ends and neighbours": np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF, 1000, 1001], np.uint64),
        "one top 24 bits": np.array(sorted(set((top | rng.integers(0, 256, 200)).tolist())), np.uint64),
        "spread over the top bits": np.array(sorted(set(((rng.integers(0, 256, 200, dtype=np.uint64) << np.uint64(24)) | rng.integers(0, 4, 200, dtype=np.uint64)).tolist())), np.uint64),
    }
    for name, keys in sets.items():
        log_table = int(np.ceil(np.log2(len(keys)))) + 1
        table, valid, keys = make_table(rng, key_bits, log_table, "half", keys=keys)
        uses = [make_use(rng, key_bits, keys, 12, False, stray=0), make_use(rng, key_bits, keys, 9, True, stray=0)]
        got, missing = check(be, uses, table, valid, key_bits)
        assert not missing, name
    # looked-up keys just below the smallest, just above the largest and between two neighbours: missing, the smallest (use, position) named
    keys = np.array([10, 20, 21, 40, 0xFFFFFFF0], np.uint64)
    table, valid, keys = make_table(rng, key_bits, 3, "half", keys=keys)
    uses = [make_use(rng, key_bits, keys, 7, False, stray=0), make_use(rng, key_bits, keys, 13, False, stray=0)]
    for pos, absent in ((7000, 9), (6000, 0xFFFFFFF1), (5000, 22), (4000, 30)):
        for c, v in zip(uses[1][0], M.split([absent], key_bits)):
            c[pos] = v[0]
    got, missing = check(be, uses, table, valid, key_bits)
    assert missing == [(1, 4000), (1, 5000), (1, 6000), (1, 7000)]
    assert "use 1 row position 4000: (%s) is not a row of the table (4 such rows)" % ", ".join(str(int(v[0])) for v in M.split([30], key_bits)) in be.L.nx_last_error(be.ctx).decode()


# ---------------------------------------------------------------- 3. skew and 64-bit sums ----------
def test_one_key_with_weight_p_minus_1_over_a_whole_use(be):
    """2^16 rows of weight p - 1 on one key: the 64-bit sum is 2^16 (p - 1) = 2^47 - 2^16, mod p = p - 2^16"""
    rng = np.random.default_rng(9)
    key_bits = [16, 16]
    table, valid, keys = make_table(rng, key_bits, 8, "half")
    n = 1 << 16
    cols = [np.full(n, v[0], np.uint32) for v in M.split(keys[17:18], key_bits)]
    got, missing = check(be, [(cols, np.full(n, P - 1, np.uint32))], table, valid, key_bits)
    assert not missing and sorted(got.tolist())[-1] == P - (1 << 16) and np.count_nonzero(got) == 1


def test_a_ninety_percent_zero_column(be):
    rng = np.random.default_rng(10)
    key_bits = [16, 16]
    keys = np.array(sorted(set([0] + rng.integers(0, 1 << 32, 300, dtype=np.uint64).tolist())), np.uint64)
    table, valid, keys = make_table(rng, key_bits, 10, "half", keys=keys)
    n = 1 << 16
    pick = np.where(rng.random(n) < 0.9, np.uint64(0), keys[rng.integers(0, len(keys), n)])
    w = rng.choice(np.array([0, 1, P - 1, P - 2], np.uint32), n)
    got, missing = check(be, [(M.split(pick, key_bits), w), (M.split(pick[::-1].copy(), key_bits), None)], table, valid, key_bits)
    assert not missing


# ---------------------------------------------------------------- 4. missing and out-of-range rows ----------
def test_missing_and_out_of_range_rows(be):
    rng = np.random.default_rng(11)
    key_bits = [16, 16]
    table, valid, keys = make_table(rng, key_bits, 9, "half")
    uses = [make_use(rng, key_bits, keys, 6, False, stray=0), make_use(rng, key_bits, keys, 13, False, stray=0), make_use(rng, key_bits, keys, 3, False, stray=0)]
    uses[1][0][1][4321] = 70000                                   # one entry outside its 16 bits: named with its value, the rest is counted
    want, missing = M.multiplicities(uses, table, valid, key_bits)
    assert missing == [(1, 4321)]
    got, res, rc = run(be, uses, table, valid, key_bits)
    assert rc == NX_ERR_PROTOCOL and res == (1, 1, 4321) and np.array_equal(got, want) and got.any()
    assert "use 1 row position 4321: (%d, 70000) is not a row of the table (1 such row)" % int(uses[1][0][0][4321]) in be.L.nx_last_error(be.ctx).decode()
    uses[2][0][0][5] = (int(uses[2][0][0][5]) + 1) & 0xFFFF      # a second missing row in a later use: the smaller (use, position) is named
    uses[0][0][0][63] = 1 << 16
    check(be, uses, table, valid, key_bits)
    got, res, rc = run(be, uses, table, valid, key_bits)
    assert res[1:] == (0, 63) and res[0] in (2, 3)
    # rows of weight 0 are never missing, whatever they hold
    w = [np.ones(len(u[0][0]), np.uint32) for u in uses]
    w[0][63], w[1][4321], w[2][5] = 0, 0, 0
    got, missing = check(be, [(u[0], x) for u, x in zip(uses, w)], table, valid, key_bits)
    assert not missing


# ---------------------------------------------------------------- 5. refusals ----------
def test_refusals_leave_the_context_usable(be, nz):
    rng = np.random.default_rng(12)
    key_bits = [16, 16]
    table, valid, keys = make_table(rng, key_bits, 8, "half")
    uses = [make_use(rng, key_bits, keys, 9, True, stray=0)]
    rows = np.flatnonzero(valid)
    a, b, c = int(rows[3]), int(rows[40]), int(rows[41])
    dup = [t.copy() for t in table]                               # two more valid rows with the key of row a
    for t in dup:
        t[b], t[c] = t[a], t[a]
    far = [t.copy() for t in table]                               # a valid table value outside its bits
    far[1][a] = 1 << 16
    d_use = be.columns_from_host(np.stack(uses[0][0] + [uses[0][1]]))
    good = be.columns_from_host(np.stack(table + [valid] + dup + far))
    up, gp = _ptrs(d_use, 3), _ptrs(good, 7)
    out = be.columns(1, 8)
    dev_use = [(up[:2], up[2], 9)]
    be.sync()
    live0, _ = be.memory()

    def still_fine():
        assert be.memory()[0] == live0
        assert be.logup_multiplicities_sparse(dev_use, gp[:2], gp[2], 8, key_bits, out.ptr.value) == (0, 0, 0)
        assert np.array_equal(out.to_cpu().reshape(-1), M.multiplicities(uses, table, valid, key_bits)[0])
        assert be.memory()[0] == live0

    still_fine()
    # two valid rows with one key: the smallest position whose key also lies at a smaller valid position, and that position
    lo, hi = int(dup[0][a]), int(dup[1][a])
    with pytest.raises(nz.NexusHipError, match=r"error -2: .*table row positions %d and %d hold the same key \(%d, %d\)" % (a, b, lo, hi)):
        be.logup_multiplicities_sparse(dev_use, gp[3:5], gp[2], 8, key_bits, out.ptr.value)
    still_fine()
    with pytest.raises(M.TableRefused) as e:
        M.multiplicities(uses, dup, valid, key_bits)
    assert (e.value.kind, e.value.first, e.value.second, e.value.entries) == ("duplicate", a, b, (lo, hi))
    with pytest.raises(nz.NexusHipError, match=r"error -2: .*table row position %d holds a value outside its key_bits" % a):
        be.logup_multiplicities_sparse(dev_use, gp[5:7], gp[2], 8, key_bits, out.ptr.value)
    still_fine()
    # key widths and counts
    for bits, match in (([16, 17], "add up to more than 32"), ([0], "key_bits of 1 to 32"), ([33], "key_bits of 1 to 32"), ([8] * 5, "1 to 4 key columns")):
        with pytest.raises(nz.NexusHipError, match=r"error -2: .*" + match):
            be.logup_multiplicities_sparse([(up[:1] * len(bits), None, 9)], gp[:1] * len(bits), None, 8, bits, out.ptr.value)
        still_fine()
    with pytest.raises(nz.NexusHipError, match=r"error -2"):
        be.logup_multiplicities_sparse([], [], None, 8, [], out.ptr.value)
    still_fine()
    with pytest.raises(nz.NexusHipError, match=r"error -2: .*log_table of 31"):
        be.logup_multiplicities_sparse(dev_use, gp[:2], gp[2], 31, key_bits, out.ptr.value)
    still_fine()
    with pytest.raises(nz.NexusHipError, match=r"error -2: .*log_size too large"):
        be.logup_multiplicities_sparse([(up[:2], None, 31)], gp[:2], gp[2], 8, key_bits, out.ptr.value)
    still_fine()
    # NULL pointers
    for args in (([([0, up[1]], up[2], 9)], gp[:2], gp[2], out.ptr.value), (dev_use, [gp[0], 0], gp[2], out.ptr.value), (dev_use, gp[:2], gp[2], None)):
        with pytest.raises(nz.NexusHipError, match=r"error -2: .*NULL"):
            be.logup_multiplicities_sparse(args[0], args[1], args[2], 8, key_bits, args[3])
        still_fine()
    # d_mult equal to an input column
    for alias in (up[0], up[2], gp[1], gp[2]):
        with pytest.raises(nz.NexusHipError, match=r"error -2: .*d_mult has the pointer of an input column"):
            be.logup_multiplicities_sparse(dev_use, gp[:2], gp[2], 8, key_bits, alias)
        still_fine()
    assert np.array_equal(good.to_cpu(), np.stack(table + [valid] + dup + far)) and np.array_equal(d_use.to_cpu(), np.stack(uses[0][0] + [uses[0][1]]))


# ---------------------------------------------------------------- 6. memory and determinism ----------
def _bound(nz, log_table, n_uses):
    """DEVICE MEMORY of include/nexus_hip.h"""
    t = 1 << log_table
    return 16 * t + 1024 * min(256, -(-t // 1024)) + 52 * n_uses + (4 << nz.MULT_SPARSE_LDS_LOG_KEYS) + 4096


def test_memory_follows_the_table_rows_not_the_key_space(be, nz):
    rng = np.random.default_rng(13)
    log_table = 13
    table, valid, keys = make_table(rng, [12, 12], log_table, "half")
    uses = [make_use(rng, [12, 12], keys, 16, True), make_use(rng, [12, 12], keys, 12, False), make_use(rng, [12, 12], keys, 3, False)]
    d = [be.columns_from_host(np.stack(u[0] + ([u[1]] if u[1] is not None else []))) for u in uses]
    dev_uses = [(_ptrs(x, 2), (_ptrs(x, 3)[2] if u[1] is not None else None), x.log_size) for x, u in zip(d, uses)]
    t = be.columns_from_host(np.stack(table + [valid]))
    tp = _ptrs(t, 3)
    peaks, words = [], []
    for key_bits in ([12, 12], [16, 16], [12, 12]):
        out = be.columns_from_host(np.full(1 << log_table, FILL, np.uint32))
        be.sync()
        live0, _ = be.memory(reset_peak=True)
        res, rc = be.logup_multiplicities_sparse(dev_uses, tp[:2], tp[2], log_table, key_bits, out.ptr.value, want_rc=True)
        live1, peak = be.memory()
        assert live1 == live0                                      # nothing is kept
        assert 0 < peak - live0 <= _bound(nz, log_table, len(uses))
        peaks.append(peak - live0)
        want, missing = M.multiplicities(uses, table, valid, key_bits)
        assert res == ((len(missing),) + missing[0] if missing else (0, 0, 0))
        words.append(out.to_cpu().reshape(-1))
        assert np.array_equal(words[-1], want)
    assert peaks[0] == peaks[1] == peaks[2]                          # independent of the key space
    assert np.array_equal(words[0], words[2])                        # two runs, identical words


# ---------------------------------------------------------------- 7. agreement with the dense call ----------
@pytest.mark.parametrize("key_bits", [[8, 8], [12]], ids=["bits8_8", "bits12"])
def test_word_for_word_the_dense_call_on_a_full_table(be, key_bits):
    rng = np.random.default_rng(14)
    tb = sum(key_bits)
    table = M.split(rng.permutation(1 << tb), key_bits)
    keys = np.arange(1 << tb, dtype=np.uint64)
    uses = [make_use(rng, key_bits, keys, 16, True), make_use(rng, key_bits, keys, 12, False), make_use(rng, key_bits, keys, 5, True)]
    uses[1][0][0][77] = 1 << key_bits[0]                              # one row both calls report missing
    d = [be.columns_from_host(np.stack(u[0] + ([u[1]] if u[1] is not None else []))) for u in uses]
    k = len(key_bits)
    dev_uses = [(_ptrs(x, k), (_ptrs(x, k + 1)[k] if u[1] is not None else None), x.log_size) for x, u in zip(d, uses)]
    t = be.columns_from_host(np.stack(table))
    dense, sparse = be.columns_from_host(np.full(1 << tb, FILL, np.uint32)), be.columns_from_host(np.full(1 << tb, FILL, np.uint32))
    r_dense = be.logup_multiplicities(dev_uses, _ptrs(t, k), tb, key_bits, dense.ptr.value, want_rc=True)
    r_sparse = be.logup_multiplicities_sparse(dev_uses, _ptrs(t, k), None, tb, key_bits, sparse.ptr.value, want_rc=True)
    assert r_dense == r_sparse == ((1, 1, 77), NX_ERR_PROTOCOL)
    assert np.array_equal(dense.to_cpu(), sparse.to_cpu())
    assert np.array_equal(sparse.to_cpu().reshape(-1), M.multiplicities(uses, table, None, key_bits)[0])


# ---------------------------------------------------------------- 8. placement ----------
class _Slab:
    """the arena of a placement plan on the device (tests/placement.py)"""

    def __init__(self, be, plan):
        self.be, self.arena, self.ptr = be, plan.arena, C.c_void_p()
        be._chk(be.L.nx_alloc(be.ctx, C.c_size_t(self.arena.size), C.byref(self.ptr)))
        assert self.ptr.value % 256 == 0
        img = self.arena.image()
        be._chk(be.L.nx_upload(be.ctx, self.ptr, img.ctypes.data_as(C.c_void_p), C.c_size_t(img.size)))

    def __call__(self, name):
        return self.ptr.value + 4 * self.arena.offset(name)

    def download(self):
        self.be.sync()
        out = np.empty(self.arena.size, np.uint32)
        self.be._chk(self.be.L.nx_download(self.be.ctx, out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.size)))
        return out


@pytest.mark.parametrize("shift", PL.SHIFTS)
@pytest.mark.parametrize("log_use,log_table", [(2, 2), (MS_TILE_LOG, 6)])
def test_columns_at_every_word_offset_between_guards(be, log_use, log_table, shift):
    rng = np.random.default_rng([log_use, shift])
    key_bits = [16, 16]
    table, valid, keys = make_table(rng, key_bits, log_table, "half")
    cols, weight = make_use(rng, key_bits, keys, log_use, True, stray=0)
    second = make_use(rng, key_bits, keys, max(log_use - 1, 0), False, stray=0)[0]
    sh = PL.Shifts(shift)
    p = PL.Plan()
    for k in range(2):
        p.add(f"table{k}", table[k], shift=sh.word())
    p.add("valid", valid, shift=sh.word())
    for k in range(2):
        p.add(f"val{k}", cols[k], shift=sh.word())
    p.add("weight", weight, shift=sh.word())
    for k in range(2):
        p.add(f"second{k}", second[k], shift=sh.word())
    p.add("mult", words=1 << log_table, shift=sh.word())
    want, missing = M.multiplicities([(cols, weight), (second, None)], table, valid, key_bits)
    assert not missing
    p.want("mult", want)
    A = _Slab(be, p)
    try:
        uses = [([A("val0"), A("val1")], A("weight"), log_use), ([A("second0"), A("second1")], None, max(log_use - 1, 0))]
        assert be.logup_multiplicities_sparse(uses, [A("table0"), A("table1")], A("valid"), log_table, key_bits, A("mult")) == (0, 0, 0)
        errs = p.arena.check(A.download(), p.expect)
        assert not errs, "\n".join(errs)
    finally:
        be.L.nx_free(be.ctx, A.ptr)


# ---------------------------------------------------------------- 9. the statement ----------
# Component ram, 2^6 rows: is_load, is_store (exclusive flags, both 0 on padding rows) and the two 16-bit limbs of a 32-bit address;
# + is_load / rel_read(addr) + is_store / rel_write(addr).  Component boundary, 2^5 rows, one per touched address: is_real, the limbs,
# mult_read, mult_write; (1 - is_real) mult_* = 0 (private_memory/mod.rs:318-320), - mult_read / rel_read(addr) - mult_write /
# rel_write(addr) (:249-262).  Everything but ram's four seed columns is made on the device.
LOG_R, LOG_B = 6, 5
TREE_LOGS = [[LOG_B], [LOG_R] * 4 + [LOG_B] * 5, [LOG_R] * 8 + [LOG_B] * 8]


def _ram_seed():
    rng = np.random.default_rng(909)
    n = 1 << LOG_R
    pool = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0x80000004, 0xFFFF0000, 0xFFFF1234, 0xFFFFFFFF] + rng.integers(0, 1 << 32, 12, dtype=np.uint64).tolist(), np.uint64)
    assert len(set(pool.tolist())) == 20
    addr = pool[rng.integers(0, len(pool), n)]
    addr[:20] = pool                                                  # every address of the pool is touched
    kind = rng.integers(0, 2, n)
    is_load, is_store = (kind == 0).astype(np.uint32), (kind == 1).astype(np.uint32)
    is_load[n - 8:], is_store[n - 8:], addr[n - 8:] = 0, 0, 0         # padding rows
    order = rng.permutation(n)                                        # rows in no particular order
    return [c[order] for c in (is_load, is_store, (addr & np.uint64(0xFFFF)).astype(np.uint32), (addr >> np.uint64(16)).astype(np.uint32))]


def _host_boundary(seed):
    """the boundary component's five columns from the model: the touched addresses ascending, then padding"""
    is_load, is_store, lo, hi = seed
    acc = (is_load + is_store) != 0
    addrs = np.unique((lo[acc].astype(np.uint64) | (hi[acc].astype(np.uint64) << np.uint64(16))))
    nb = 1 << LOG_B
    b_lo, b_hi, is_real = np.zeros(nb, np.uint32), np.zeros(nb, np.uint32), np.zeros(nb, np.uint32)
    b_lo[:len(addrs)], b_hi[:len(addrs)], is_real[:len(addrs)] = M.split(addrs, [16, 16]) + [1]
    mr, miss_r = M.multiplicities([([lo, hi], is_load)], [b_lo, b_hi], is_real, [16, 16])
    mw, miss_w = M.multiplicities([([lo, hi], is_store)], [b_lo, b_hi], is_real, [16, 16])
    assert not miss_r and not miss_w and int(mr.sum()) == int(is_load.sum()) and int(mw.sum()) == int(is_store.sum())
    return [is_real, b_lo, b_hi, mr, mw]


def _ram_programs(ap, rels, shifts, only=None):
    """only: None = both relations (the statement), 0 / 1 = the read / write relation alone (its own claimed sum)"""
    pa = ap.ProgramBuilder()
    is_load, is_store, lo, hi = [pa.next_trace_mask(k)[0] for k in range(4)]
    pa.add_constraint(is_load * (is_load - 1))
    pa.add_constraint(is_store * (is_store - 1))
    pa.add_constraint(is_load * is_store)
    for k, flag in enumerate((is_load, is_store)):
        if only in (None, k):
            pa.add_to_relation(pa.relation(*rels[k], 2), flag, [lo, hi])
    pa.finalize_logup(4, shifts[0])
    pb = ap.ProgramBuilder()
    zero, is_real, lo, hi, mr, mw = [pb.next_trace_mask(k)[0] for k in range(6)]      # column 0: the preprocessed tree's one column, all zero
    pb.add_constraint(zero * is_real)
    pb.add_constraint((1 - is_real) * mr)
    pb.add_constraint((1 - is_real) * mw)
    for k, m in enumerate((mr, mw)):
        if only in (None, k):
            pb.add_to_relation(pb.relation(*rels[k], 2), -m, [lo, hi])
    pb.finalize_logup(6, shifts[1])
    return pa, pb


def _upload(be, ptr, host):
    host = np.ascontiguousarray(host, np.uint32)
    be._chk(be.L.nx_upload(be.ctx, C.c_void_p(ptr), host.ctypes.data_as(C.c_void_p), C.c_size_t(len(host))))


def _words(be, nz, ptr, log):
    return nz.DeviceColumns.view(be, ptr, 1, log).to_cpu().reshape(-1)


def _claimed(be, frac, cols, log, out=None):
    out = out if out is not None else _ptrs(be.columns(4 * frac.n_logup_cols, log), 4 * frac.n_logup_cols)
    be.logup_program(frac, cols + [None] * len(out), log, out_ptrs=out)
    return be.logup_finalize_last(out[-4:], log_size=log)


def _ram_session(be, nz, control=None):
    import nexus_zkvm_amd.air_program as ap
    cfg = nz.default_config(pow_bits=2)
    seed = _ram_seed()
    host_b = _host_boundary(seed)
    pre = np.zeros(1 << LOG_B, np.uint32)                             # a session commits a preprocessed tree first: one zero column, claimed by the boundary
    s = be.prover_session(cfg, LOG_R)
    s.mix_u64(9)
    roots = [s.commit([pre])]
    d_pre = be.columns_from_host(pre)
    main = s.tree_begin(TREE_LOGS[1])
    ram, bnd = main[:4], main[4:]
    for d, col in zip(ram, seed):
        _upload(be, d, col)
    for d in bnd:
        be._chk(be.L.nx_memset_zero(be.ctx, C.c_void_p(d), C.c_size_t(1 << LOG_B)))
    # the accesses' flag into a scratch column; the distinct addresses' limbs straight into the boundary's columns, their counts into another
    flag, skey, count = be.columns(1, LOG_R), be.columns(1, LOG_B), be.columns(1, LOG_B)
    be._chk(be.L.nx_memset_zero(be.ctx, count.ptr, C.c_size_t(1 << LOG_B)))
    tp = ap.ProgramBuilder()
    tp.store(2, tp.next_trace_mask(0)[0] + tp.next_trace_mask(1)[0])
    be.trace_program(tp.build_trace_program(), [ram[0], ram[1], flag.ptr.value], LOG_R)
    stream = {"key": [ram[2], ram[3]], "flag": flag.ptr.value, "payload": [ram[2], ram[3]], "log_size": LOG_R}
    n_keys = be.trace_prev_access([stream], [16, 16], 2, summary=(1 << LOG_B, skey.ptr.value, count.ptr.value, [bnd[1], bnd[2]]))
    assert n_keys == int(host_b[0].sum()) == 20
    tp = ap.ProgramBuilder()
    tp.store(1, 1 - tp.eq(tp.next_trace_mask(0)[0], 0))                # is_real = (count != 0)
    be.trace_program(tp.build_trace_program(), [count.ptr.value, bnd[0]], LOG_B)
    if control == "removed":                                            # one touched address taken out of the table
        gone = 7
        col = _words(be, nz, bnd[0], LOG_B)
        col[gone] = 0
        _upload(be, bnd[0], col)
        res, rc = be.logup_multiplicities_sparse([([ram[2], ram[3]], ram[0], LOG_R)], [bnd[1], bnd[2]], bnd[0], LOG_B, [16, 16], bnd[3], want_rc=True)
        is_load, _, lo, hi = seed
        hit = np.flatnonzero((is_load != 0) & (lo == host_b[1][gone]) & (hi == host_b[2][gone]))
        text = be.L.nx_last_error(be.ctx).decode()
        s.close()
        return res, rc, hit, text
    for weight, out in ((ram[0], bnd[3]), (ram[1], bnd[4])):
        assert be.logup_multiplicities_sparse([([ram[2], ram[3]], weight, LOG_R)], [bnd[1], bnd[2]], bnd[0], LOG_B, [16, 16], out) == (0, 0, 0)
    got = [_words(be, nz, d, lg) for d, lg in zip(main, TREE_LOGS[1])]
    for k, (g, h) in enumerate(zip(got, seed + host_b)):
        assert np.array_equal(g, h), "main column %d" % k
    if control == "tampered":                                           # one addr_lo word of an accessing row changed after the counts
        pos = int(np.flatnonzero(got[0] + got[1])[5])
        col = got[2].copy()
        col[pos] ^= 1
        _upload(be, ram[2], col)
    kept = [be.clone_columns(nz.DeviceColumns.view(be, d, 1, lg)) for d, lg in zip(main, TREE_LOGS[1])]      # the commit turns columns into coefficients
    roots.append(s.tree_commit())
    rels = [(s.draw_felt(), s.draw_felt()), (s.draw_felt(), s.draw_felt())]
    ins = [[k.ptr.value for k in kept[:4]], [d_pre.ptr.value] + [k.ptr.value for k in kept[4:]]]
    # each relation's two claimed sums on their own
    pairs = []
    for only in (0, 1):
        fr = [p.build_logup() for p in _ram_programs(ap, rels, [(0, 0, 0, 0)] * 2, only=only)]
        pairs.append([_claimed(be, f, cols, log) for f, cols, log in zip(fr, ins, (LOG_R, LOG_B))])
    fracs = [p.build_logup() for p in _ram_programs(ap, rels, [(0, 0, 0, 0)] * 2)]
    inter = s.tree_begin(TREE_LOGS[2])
    claimed, shifts = [], []
    for frac, cols, out, log in zip(fracs, ins, [inter[:8], inter[8:]], (LOG_R, LOG_B)):
        assert 4 * frac.n_logup_cols == len(out)
        claimed.append(_claimed(be, frac, cols, log, out))
        n_inv = pow((1 << log) % P, P - 2, P)
        shifts.append([(int(x) * n_inv) % P for x in claimed[-1]])
    claimed = np.array(claimed, np.uint32)
    if control == "tampered":
        s.close()
        return pairs, claimed
    s.mix_felts(claimed)
    roots.append(s.tree_commit())
    pa, pb = _ram_programs(ap, rels, shifts)
    comps = [ap.Component(LOG_R, pa.build(), [(1, k) for k in range(4)] + [(2, k) for k in range(8)]),
             ap.Component(LOG_B, pb.build(), [(0, 0)] + [(1, 4 + k) for k in range(5)] + [(2, 8 + k) for k in range(8)])]
    return pairs, claimed, (s, cfg, comps, roots, rels, seed + host_b, pre)


def _cancel(sums):
    return [int(sum(int(c[q]) for c in sums) % P) for q in range(4)] == [0, 0, 0, 0]


def test_a_read_write_address_statement_filled_on_the_device_is_proved_and_verified(be, nz):
    pairs, claimed, (s, cfg, comps, roots, rels, host_main, pre) = _ram_session(be, nz)
    for pair in pairs:                                                  # reads against MultiplicityRead, writes against MultiplicityWrite
        assert _cancel(pair) and all(c.any() for c in pair)
    assert _cancel(claimed) and all(c.any() for c in claimed)
    report = s.check(comps)
    assert report.ok, report
    words = s.prove(comps)
    v = nz.VerifierSession(cfg)
    v.mix_u64(9)
    v.commit(roots[0], TREE_LOGS[0])
    v.commit(roots[1], TREE_LOGS[1])
    for z, alpha in rels:
        assert np.array_equal(v.draw_felt(), z) and np.array_equal(v.draw_felt(), alpha)
    v.mix_felts(claimed)
    v.commit(roots[2], TREE_LOGS[2])
    assert v.verify(comps, words) is None
    assert np.array_equal(v.digest(), s.digest())
    s.close()
    # the same main tree from a session fed the model's columns by the host: byte-equal root
    h = be.prover_session(cfg, LOG_R)
    h.mix_u64(9)
    assert np.array_equal(h.commit([pre]), roots[0])
    for d, col in zip(h.tree_begin(TREE_LOGS[1]), host_main):
        _upload(be, d, col)
    assert np.array_equal(h.tree_commit(), roots[1])
    h.close()


def test_controls_of_the_statement(be, nz):
    # one addr_lo word of an accessing row changed after the counts: the sums no longer cancel
    pairs, claimed = _ram_session(be, nz, control="tampered")
    assert not _cancel(claimed) and not (_cancel(pairs[0]) and _cancel(pairs[1]))
    # an access to an address removed from the table: NX_ERR_PROTOCOL naming its use and position
    res, rc, hit, text = _ram_session(be, nz, control="removed")
    assert len(hit) and rc == NX_ERR_PROTOCOL and res == (len(hit), 0, int(hit[0]))
    assert "use 0 row position %d: " % int(hit[0]) in text and "is not a row of the table" in text
