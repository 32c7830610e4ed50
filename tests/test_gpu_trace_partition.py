"""nx_trace_partition_create / nx_trace_partition_fill on the device against the model of tests/trace_partition_model.py (a stable
argsort, the coset row of a position from the definition, limbs cut from integers).  Every comparison is an equality of words.
1. every size around a tile edge x 1 / 3 / 40 / 256 classes, destinations for every class and for all steps, every limb shape, the
   optional outputs on and off; one table above 2^20 steps, where a block of the counting pass takes more than its four tiles;
2. skew;  3. refused class words and every NX_ERR_ARG of the fill;  4. determinism and memory;
5. a v2-shaped statement made from a step table on the device, proved and verified.  It is the PROGRAM-EXECUTION relation only
   (rel-cont-prog-exec of the reference's prover2): the decoding, program-memory, register-memory and range-check relations of the
   components are left out, so nothing here ties an opcode to an instruction word."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import trace_partition_model as M

pytestmark = pytest.mark.gpu
P = M.P
NX_OK, NX_ERR_ARG, NX_ERR_PROTOCOL = 0, -2, -4
GUARD = 0xDEADBEEF
# (src, shift, bits): bytes and half-words, an unaligned six-bit field, the lowest and the highest bit, 31 bits from bit 0 (source 2
# holds words equal to p, written as 0) and from bit 1, and source 3 read by six specs
SPECS = [(0, 0, 8), (0, 8, 8), (0, 16, 16), (1, 2, 6), (1, 0, 1), (1, 31, 1), (2, 0, 31), (2, 1, 31),
         (3, 0, 8), (3, 8, 8), (3, 16, 8), (3, 24, 8), (3, 0, 16), (3, 16, 16)]
N_SRC = 4


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


def _upload(be, ptr, host):
    host = np.ascontiguousarray(host, np.uint32)
    if len(host):
        be._chk(be.L.nx_upload(be.ctx, C.c_void_p(ptr), host.ctypes.data_as(C.c_void_p), C.c_size_t(len(host))))


def _words(be, nz, host):
    """a linear device array of exactly these words (a step-table column); keep the returned object alive"""
    host = np.ascontiguousarray(host, np.uint32)
    d = nz.DeviceColumns(be, 1, max(0, int(len(host) - 1).bit_length()))
    _upload(be, d.ptr.value, host)
    return d


def make_sources(rng, n):
    src = [rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) for _ in range(N_SRC)]
    src[2][::3] = P
    if n > 1:
        src[2][1] = 0xFFFFFFFF
    return src


class Table:
    def __init__(self, be, nz, cls, src):
        self.be, self.nz, self.cls, self.src, self.n = be, nz, np.asarray(cls, np.uint32), src, len(cls)
        self.d_cls = _words(be, nz, self.cls)
        self.d_src = [_words(be, nz, s) for s in src]
        self.src_ptrs = [d.ptr.value for d in self.d_src]

    def create(self, n_classes, want_rc=False):
        return self.be.trace_partition(self.d_cls.ptr.value if self.n else None, self.n, n_classes, want_rc=want_rc)


class Outputs:
    """the columns of one destination as a slab filled with a guard word: its limb columns, is_pad, step, and one column behind them
    that nothing may write"""

    def __init__(self, be, nz, dest):
        self.dest, self.log, self.nc = dest, dest["log_size"], len(dest["limbs"])
        self.slab = nz.DeviceColumns(be, self.nc + 3, self.log).upload(np.full((self.nc + 3, 1 << self.log), GUARD, np.uint32))
        ptr = lambda i: self.slab.ptr.value + i * (4 << self.log)
        self.arg = {"cls": dest["cls"], "log_size": self.log, "cols": [ptr(i) for i in range(self.nc)], "limbs": dest["limbs"],
                    "is_pad": ptr(self.nc) if dest["is_pad"] else None, "step": ptr(self.nc + 1) if dest["step"] else None}

    def read(self):
        return self.slab.to_cpu()

    def check(self, want, tag):
        got = self.read()
        for c in range(self.nc):
            assert np.array_equal(got[c], want["cols"][c]), (tag, "column", c, self.dest["limbs"][c])
        guard = np.full(1 << self.log, GUARD, np.uint32)
        assert np.array_equal(got[self.nc], want["is_pad"] if self.dest["is_pad"] else guard), (tag, "is_pad")
        assert np.array_equal(got[self.nc + 1], want["step"] if self.dest["step"] else guard), (tag, "step")
        assert np.array_equal(got[self.nc + 2], guard), (tag, "the column behind the outputs was written")


def make_dests(counts, n_steps, n_classes, few_specs):
    """every class, all steps, and class 0 a second time; the log_size rotates through the helper's value with min_log 1 and 4 and two
    sizes above it, the optional outputs through their four combinations"""
    dests = []
    for i in range(n_classes + 2):
        cls = i if i < n_classes else M.ALL if i == n_classes else 0
        count = n_steps if cls == M.ALL else int(counts[cls])
        log = [M.log_size(count, 1), M.log_size(count, 4), M.log_size(count, 1) + 1, M.log_size(count, 4) + 2][i % 4]
        limbs = [SPECS[(i + k) % len(SPECS)] for k in range(1 + i % 5)] if few_specs and cls != M.ALL else list(SPECS)
        dests.append({"cls": cls, "log_size": log, "limbs": limbs, "is_pad": bool(i & 1) or cls == M.ALL, "step": bool(i & 2) or cls == M.ALL})
    return dests


def run(be, nz, cls, n_classes, src, dests=None, few_specs=False):
    want_counts, steps_of = M.partition(cls, n_classes)
    t = Table(be, nz, cls, src)
    counts, part = t.create(n_classes)
    try:
        assert np.array_equal(counts, want_counts)
        for c in counts:
            assert nz.partition_log_size(int(c), 4) == M.log_size(int(c), 4)
        dests = dests or make_dests(counts, t.n, n_classes, few_specs)
        outs = [Outputs(be, nz, d) for d in dests]
        part.fill(t.src_ptrs, [o.arg for o in outs])
        for i, o in enumerate(outs):
            o.check(M.fill(cls, n_classes, src, o.dest, steps_of), "destination %d" % i)
    finally:
        part.destroy()
    return counts


def classes(rng, n, k, with_none):
    cls = rng.integers(0, k, size=n, dtype=np.uint32)
    if with_none:
        cls[rng.random(n) < 0.2] = M.NONE
    return cls


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 5, (1 << 17) + 3]      # 256: a fill tile; 1024: four tiles, an order block
N_CLASSES = [1, 3, 40, 256]


@pytest.mark.parametrize("n_classes", N_CLASSES)
@pytest.mark.parametrize("n_steps", SIZES)
def test_exact_against_the_model(be, nz, n_steps, n_classes):
    v = SIZES.index(n_steps) * len(N_CLASSES) + N_CLASSES.index(n_classes)
    rng = np.random.default_rng(7100 + v)
    run(be, nz, classes(rng, n_steps, n_classes, with_none=v % 3 == 1), n_classes, make_sources(rng, n_steps), few_specs=n_classes > 3)


def test_a_block_of_the_counting_pass_takes_more_than_its_four_tiles(be, nz):
    """up to 2^20 steps an order block takes four tiles of 256 steps; 2^20 + 2^10 + 1 steps make it five on 1024 blocks"""
    rng = np.random.default_rng(7171)
    n = (1 << 20) + (1 << 10) + 1
    cls = classes(rng, n, 3, with_none=True)
    src = make_sources(rng, n)
    counts = M.partition(cls, 3)[0]
    dests = [{"cls": c, "log_size": M.log_size(int(counts[c]), 4), "limbs": [SPECS[0], SPECS[6], SPECS[13]], "is_pad": c == 1, "step": True} for c in range(3)]
    dests.append({"cls": M.ALL, "log_size": 21, "limbs": [SPECS[3], SPECS[7]], "is_pad": True, "step": True})
    run(be, nz, cls, 3, src, dests=dests)


def _skewed(name, rng, n, k):
    j = np.arange(n, dtype=np.uint32)
    if name == "one_class":
        return np.full(n, k - 1, np.uint32)
    if name == "all_but_one":
        cls = np.full(n, k - 1, np.uint32)
        cls[n // 2] = 0
        return cls
    if name == "absent_classes":
        return np.where(rng.random(n) < 0.5, 0, (k - 1) // 2).astype(np.uint32)
    if name == "sorted":
        return np.sort(rng.integers(0, k, size=n, dtype=np.uint32))
    if name == "alternating":
        return np.where(j & 1, k - 1, 0).astype(np.uint32)
    if name == "runs_of_64":
        return ((j // 64) % k).astype(np.uint32)
    if name == "runs_of_65":
        return ((j // 65) % k).astype(np.uint32)
    if name == "none_mixed_in":
        return classes(rng, n, k, with_none=True)
    assert name == "all_none"
    return np.full(n, M.NONE, np.uint32)


@pytest.mark.parametrize("name", ["one_class", "all_but_one", "absent_classes", "sorted", "alternating", "runs_of_64", "runs_of_65", "none_mixed_in", "all_none"])
def test_skew(be, nz, name):
    rng = np.random.default_rng(72)
    for n in (1500, 4 * 1024 + 1):
        counts = run(be, nz, _skewed(name, rng, n, 2 if name == "alternating" else 5), 2 if name == "alternating" else 5, make_sources(rng, n))
        if name == "one_class":
            assert counts.tolist() == [0, 0, 0, 0, n]
        if name == "all_none":
            assert not counts.any()


@pytest.mark.parametrize("k", [0, 1, 9, 12])
def test_a_class_of_exactly_a_power_of_two_and_one_more(be, nz, k):
    """2^k steps: no padding row at all; 2^k + 1: the next size, almost nothing but padding"""
    rng = np.random.default_rng(73 + k)
    for count in ((1 << k), (1 << k) + 1):
        n = 3 * count + 7
        cls = np.full(n, 1, np.uint32)
        cls[rng.permutation(n)[:count]] = 0
        src = make_sources(rng, n)
        log = M.log_size(count, 1)
        assert log == (max(k, 1) if count == 1 << k else k + 1)
        run(be, nz, cls, 2, src, dests=[{"cls": 0, "log_size": log, "limbs": list(SPECS), "is_pad": True, "step": True}])


@pytest.mark.parametrize("bad_word", [40, 0xFFFFFFFE])
def test_a_class_word_outside_the_classes_is_refused(be, nz, bad_word):
    rng = np.random.default_rng(74)
    n, k = 5000, 40
    cls = classes(rng, n, k, with_none=True)
    cls[[4321, 1717, 1718]] = [bad_word, bad_word, k + 7]
    assert M.first_bad(cls, k) == (1717, bad_word)
    t = Table(be, nz, cls, make_sources(rng, n))
    be.sync()
    live0, _ = be.memory()
    counts, part, rc = t.create(k, want_rc=True)
    assert rc == NX_ERR_PROTOCOL and counts is None and part is None
    msg = be.L.nx_last_error(be.ctx).decode()
    assert msg == "nx_trace_partition_create: step 1717: class %d, 40 classes" % bad_word, msg
    assert be.memory()[0] == live0
    with pytest.raises(nz.NexusHipError):
        t.create(k)
    assert be.memory()[0] == live0
    cls[[4321, 1717, 1718]] = [0, M.NONE, 39]                          # the same context partitions a good table
    run(be, nz, cls, k, t.src, few_specs=True)


def test_every_bad_argument_of_the_fill_launches_nothing(be, nz):
    rng = np.random.default_rng(75)
    n, k = 300, 3
    cls = classes(rng, n, k, with_none=False)
    t = Table(be, nz, cls, make_sources(rng, n))
    counts, part = t.create(k)
    other = nz.HipBackend(0)

    def refused(text, change, src_ptrs=None, backend=None):
        dests = [{"cls": 0, "log_size": 9, "limbs": [(0, 0, 8), (1, 8, 8)], "is_pad": True, "step": True}, {"cls": M.ALL, "log_size": 9, "limbs": [(1, 0, 31)], "is_pad": False, "step": False}]
        outs = [Outputs(be, nz, d) for d in dests]
        args = [dict(o.arg) for o in outs]
        ptrs = list(t.src_ptrs) if src_ptrs is None else src_ptrs
        change(args, ptrs)
        b = backend or be
        part.be = b
        try:
            rc = part.fill(ptrs, args, want_rc=True)
        finally:
            part.be = be
        msg = b.L.nx_last_error(b.ctx).decode()
        assert rc == NX_ERR_ARG and msg.startswith("nx_trace_partition_fill: ") and text in msg, (rc, msg, text)
        be.sync()
        for o in outs:
            assert (o.read() == GUARD).all(), text

    try:
        refused("another context", lambda a, s: None, backend=other)
        refused("destination 0: class 3, 3 classes", lambda a, s: a[0].update(cls=3))
        refused("destination 0: class 4294967294, 3 classes", lambda a, s: a[0].update(cls=0xFFFFFFFE))
        refused("destination 0: log_size of 0", lambda a, s: a[0].update(log_size=0))
        refused("destination 1: log_size of 31", lambda a, s: a[1].update(log_size=31))
        refused("destination 1: log_size of 8, its 300 steps do not fit 2^8", lambda a, s: a[1].update(log_size=8))
        small = M.log_size(int(counts[0]), 1) - 1
        refused("destination 0: log_size of %d, its %d steps do not fit" % (small, counts[0]), lambda a, s: a[0].update(log_size=small))
        refused("destination 0 column 1: src of 4, 4 source columns", lambda a, s: a[0].update(limbs=[(0, 0, 8), (4, 8, 8)]))
        refused("destination 0 column 0: shift 0 bits 0", lambda a, s: a[0].update(limbs=[(0, 0, 0), (1, 8, 8)]))
        refused("destination 0 column 0: shift 0 bits 32", lambda a, s: a[0].update(limbs=[(0, 0, 32), (1, 8, 8)]))
        refused("destination 0 column 1: shift 25 bits 8", lambda a, s: a[0].update(limbs=[(0, 0, 8), (1, 25, 8)]))
        refused("destination 0 column 1: shift 32 bits 1", lambda a, s: a[0].update(limbs=[(0, 0, 8), (1, 32, 1)]))
        refused("destination 0 column 1: NULL output column", lambda a, s: a[0].update(cols=[a[0]["cols"][0], None]))
        refused("destination 0 column 1: d_src[1] is NULL", lambda a, s: s.__setitem__(1, None))
        refused("has the pointer of destination 0 column 0", lambda a, s: a[0].update(cols=[a[0]["cols"][0], a[0]["cols"][0]]))
        refused("has the pointer of destination 0 column 1", lambda a, s: a[1].update(cols=[a[0]["cols"][1]]))
        refused("has the pointer of", lambda a, s: a[0].update(step=a[0]["is_pad"]))
        refused("has the pointer of", lambda a, s: a[1].update(is_pad=a[0]["cols"][0]))
        refused("has the pointer of a source or class column", lambda a, s: a[0].update(step=t.src_ptrs[3]))
        refused("has the pointer of a source or class column", lambda a, s: a[0].update(is_pad=t.d_cls.ptr.value))
    finally:
        part.destroy()
        other.close()
    # the refusals of create that want a context
    for kw, text in ((dict(n_classes=0), "n_classes of 0"), (dict(n_classes=257), "n_classes of 257"), (dict(n_steps=(1 << 30) + 1), "n_steps of 1073741825")):
        a = dict(n_steps=n, n_classes=k)
        a.update(kw)
        assert be.trace_partition(t.d_cls.ptr.value, a["n_steps"], a["n_classes"], want_rc=True) == (None, None, NX_ERR_ARG)
        assert text in be.L.nx_last_error(be.ctx).decode()
    assert be.trace_partition(None, n, k, want_rc=True) == (None, None, NX_ERR_ARG) and "NULL d_class" in be.L.nx_last_error(be.ctx).decode()


def test_same_words_on_two_runs_and_nothing_kept(be, nz):
    rng = np.random.default_rng(76)
    n, k = (1 << 16) + 77, 40
    cls = classes(rng, n, k, with_none=True)
    t = Table(be, nz, cls, make_sources(rng, n))
    be.sync()
    live0, _ = be.memory(reset_peak=True)
    counts, part = t.create(k)
    live1, peak = be.memory()
    order_bytes = (4 * n + 255) & ~255
    assert live1 - live0 == order_bytes                                # the order alone stays
    assert order_bytes < peak - live0 <= order_bytes + 4 * k * 1024 + 1280 + 512        # the bound of include/nexus_hip.h
    dests = make_dests(counts, n, k, few_specs=True)
    a, b = [Outputs(be, nz, d) for d in dests], [Outputs(be, nz, d) for d in dests]
    live2 = be.memory()[0]
    part.fill(t.src_ptrs, [o.arg for o in a])
    assert be.memory()[0] == live2                                     # the fill allocates nothing
    counts2, part2 = t.create(k)
    part2.fill(t.src_ptrs, [o.arg for o in b])
    assert np.array_equal(counts, counts2)
    for x, y in zip(a, b):
        assert np.array_equal(x.read(), y.read())
    part2.destroy()
    part.destroy()
    for o in a + b:
        o.slab.free()
    assert be.memory()[0] == live0


# ---------------------------------------------------------------- 5. a v2-shaped statement from a step table ----------
# The step table has the columns class, pc, clk, b, c and the execution's result a (ADD: b + c, SUB: b - c; the third class, NOP, only
# advances pc and clk).  pc starts at 0xFFF0 and grows by 4, so the fifth step's successor crosses the 16-bit boundary and PcCarry is 1
# on exactly one row of one component; clk = step + 1.
# Components (reference prover2/machine/src/components):
#   cpu       every step, NX_PART_ALL.  Preprocessed Clk low / high = row + 1; main IsPad, PcAux = pc[7:2], PcNext8_15, PcHigh, all from
#             the fill.  consume(rel-cont-prog-exec, 1 - is-pad, (clk, pc)): numerator is_pad - 1 (cpu/mod.rs:124-147).
#   add, sub  execution/add/columns.rs (Clk 2, ClkCarry, AVal 4, BVal 4, Pc 2, PcCarry, IsLocalPad, HCarry 2) + the four c-val bytes.
#             Clk, BVal, CVal, Pc, IsLocalPad from the fill; ClkCarry, PcCarry, AVal, HCarry / HBorrow from nx_trace_program on the
#             component's own columns.  ClkIncrement, PcIncrement (utils/constraints.rs:10-60), the two 16-bit sum constraints
#             (execution/add/mod.rs:256-282) and their sub counterparts; provide(rel-cont-prog-exec, 1 - is-local-pad, (clk-next,
#             pc-next)) (execution/common/mod.rs:156-166).  The reference writes the next low limb as `pc[0] + 4 - pc_carry`; that
#             balances only while no carry occurs.  This table crosses the boundary, so the carry is taken with its weight 2^16 here.
#   nop       Clk, ClkCarry, Pc, PcCarry, IsLocalPad: the two increments and the same provide.
#   boundary  cpu_boundary/mod.rs: provides the first (clk, pc), consumes the last (clk-next, pc-next).
# A step labelled with another opcode is still a step of exactly one component, and with every derived column computed from the
# component's own seeds it would be a VALID step of that opcode: in this reduced statement only the execution's own result can give it
# away.  The mislabelling control therefore takes AVal from the table's result column (limb specs of the same fill) instead of from the
# trace program; everything else is the flow of the main test.
ADD, SUB, NOP = 0, 1, 2
N_EXEC, PC0, MIN_LOG = 200, 0xFFF0, 4
S_PC, S_CLK, S_B, S_C, S_A = range(5)
EXEC_COLS, NOP_COLS = 21, 7
CLK, CLK_CARRY, AVAL, BVAL, PC, PC_CARRY, PAD, HCARRY, CVAL = 0, 2, 3, 7, 11, 13, 14, 15, 17
KIND = ["add", "sub", "nop"]


def _execution(mislabel):
    rng = np.random.default_rng(77)
    true_cls = rng.integers(0, 3, size=N_EXEC, dtype=np.uint32)
    pc = (PC0 + 4 * np.arange(N_EXEC)).astype(np.uint32)
    clk = (np.arange(N_EXEC) + 1).astype(np.uint32)
    b = rng.integers(0, 1 << 32, size=N_EXEC, dtype=np.uint64)
    c = rng.integers(0, 1 << 32, size=N_EXEC, dtype=np.uint64)
    victim = int(np.flatnonzero(true_cls == ADD)[9])
    c[victim] = 0x12345678
    a = np.where(true_cls == ADD, b + c, np.where(true_cls == SUB, b - c, 0)) & np.uint64(0xFFFFFFFF)
    cls = true_cls.copy()
    if mislabel:
        cls[victim] = SUB
    return {"cls": cls, "src": [pc, clk, b.astype(np.uint32), c.astype(np.uint32), a.astype(np.uint32)], "victim": victim}


def _bytes(src):
    return [(src, 8 * j, 8) for j in range(4)]


def _exec_limbs(kind, aval_from_table):
    """column index -> limb spec, for the columns the fill writes"""
    if kind == "nop":
        return {0: (S_CLK, 0, 16), 1: (S_CLK, 16, 16), 3: (S_PC, 0, 16), 4: (S_PC, 16, 16)}
    m = {CLK: (S_CLK, 0, 16), CLK + 1: (S_CLK, 16, 16), PC: (S_PC, 0, 16), PC + 1: (S_PC, 16, 16)}
    for j in range(4):
        m[BVAL + j], m[CVAL + j] = _bytes(S_B)[j], _bytes(S_C)[j]
        if aval_from_table:
            m[AVAL + j] = _bytes(S_A)[j]
    return m


def _derive_program(ap, kind, aval_from_table):
    """ClkCarry, PcCarry and (add, sub) AVal, HCarry / HBorrow from the component's own Clk, Pc, BVal and CVal columns"""
    tp = ap.ProgramBuilder()
    ld = lambda k: tp.next_trace_mask(k)[0]
    if kind == "nop":
        tp.store(2, tp.shr(ld(0) + 1, 16))
        tp.store(5, tp.shr(ld(3) + 4, 16))
        return tp.build_trace_program()
    tp.store(CLK_CARRY, tp.shr(ld(CLK) + 1, 16))
    tp.store(PC_CARRY, tp.shr(ld(PC) + 4, 16))
    bv, cv = [ld(BVAL + j) for j in range(4)], [ld(CVAL + j) for j in range(4)]
    b_lo, b_hi, c_lo, c_hi = bv[0] + bv[1] * 256, bv[2] + bv[3] * 256, cv[0] + cv[1] * 256, cv[2] + cv[3] * 256
    if kind == "add":
        lo = b_lo + c_lo
        h1 = tp.shr(lo, 16)
        hi = b_hi + c_hi + h1
        h2 = tp.shr(hi, 16)
    else:
        lo = b_lo + 65536 - c_lo
        h1 = 1 - tp.shr(lo, 16)                                        # the borrow
        hi = b_hi + 65536 - c_hi - h1
        h2 = 1 - tp.shr(hi, 16)
    tp.store(HCARRY, h1)
    tp.store(HCARRY + 1, h2)
    if not aval_from_table:
        for j, half in enumerate((lo, lo, hi, hi)):
            tp.store(AVAL + j, tp.band(tp.shr(half, 8 * (j & 1)), 255))
    return tp.build_trace_program()


def _host_derived(kind, cols):
    """the same derivation on the host, over storage-order columns (a dict column -> array), for the model's session"""
    u = lambda k: cols[k].astype(np.int64)
    if kind == "nop":
        cols[2], cols[5] = ((u(0) + 1) >> 16).astype(np.uint32), ((u(3) + 4) >> 16).astype(np.uint32)
        return
    cols[CLK_CARRY], cols[PC_CARRY] = ((u(CLK) + 1) >> 16).astype(np.uint32), ((u(PC) + 4) >> 16).astype(np.uint32)
    b_lo, b_hi, c_lo, c_hi = u(BVAL) + 256 * u(BVAL + 1), u(BVAL + 2) + 256 * u(BVAL + 3), u(CVAL) + 256 * u(CVAL + 1), u(CVAL + 2) + 256 * u(CVAL + 3)
    if kind == "add":
        lo = b_lo + c_lo
        h1 = lo >> 16
        hi = b_hi + c_hi + h1
        h2 = hi >> 16
    else:
        lo = b_lo + 65536 - c_lo
        h1 = 1 - (lo >> 16)
        hi = b_hi + 65536 - c_hi - h1
        h2 = 1 - (hi >> 16)
    cols[HCARRY], cols[HCARRY + 1] = h1.astype(np.uint32), h2.astype(np.uint32)
    for j, half in enumerate((lo, lo, hi, hi)):
        cols[AVAL + j] = ((half >> (8 * (j & 1))) & 255).astype(np.uint32)


def _programs(ap, z, alpha, shifts):
    """the five components' constraints and relation entries, restated with the recorder; the execution components' constraint order is
    the reference's: ClkIncrement, PcIncrement, first sum, second sum, then the logup column"""
    out = []
    cpu = ap.ProgramBuilder()
    clk_lo, clk_hi, is_pad, pc_aux, pc8, pc_high = [cpu.next_trace_mask(k)[0] for k in range(6)]
    rel = cpu.relation(z, alpha, 4)
    cpu.add_to_relation(rel, is_pad - 1, [clk_lo, clk_hi, pc_aux * 4 + pc8 * 256, pc_high])
    cpu.finalize_logup(6, shifts[0])
    out.append(cpu)
    for i, kind in enumerate(KIND):
        pb = ap.ProgramBuilder()
        n_cols = NOP_COLS if kind == "nop" else EXEC_COLS
        col = [pb.next_trace_mask(k)[0] for k in range(n_cols)]
        if kind == "nop":
            clk, clk_carry, pc, pc_carry, pad = col[0:2], col[2], col[3:5], col[5], col[6]
        else:
            clk, clk_carry, pc, pc_carry, pad = col[CLK:CLK + 2], col[CLK_CARRY], col[PC:PC + 2], col[PC_CARRY], col[PAD]
        pb.add_constraint(clk_carry * (1 - clk_carry))
        clk_next = [clk[0] + 1 - clk_carry * 65536, clk[1] + clk_carry]
        pb.add_constraint(pc_carry * (1 - pc_carry))
        pc_next = [pc[0] + 4 - pc_carry * 65536, pc[1] + pc_carry]
        if kind != "nop":
            a, b, c, h = col[AVAL:AVAL + 4], col[BVAL:BVAL + 4], col[CVAL:CVAL + 4], col[HCARRY:HCARRY + 2]
            if kind == "add":       # a + carry 2^16 = b + c (+ carry in)
                pb.add_constraint((1 - pad) * (a[0] + a[1] * 256 + h[0] * 65536 - (b[0] + b[1] * 256 + c[0] + c[1] * 256)))
                pb.add_constraint((1 - pad) * (a[2] + a[3] * 256 + h[1] * 65536 - (b[2] + b[3] * 256 + c[2] + c[3] * 256 + h[0])))
            else:                   # a + c = b + borrow 2^16 (+ borrow in)
                pb.add_constraint((1 - pad) * (a[0] + a[1] * 256 + c[0] + c[1] * 256 - (b[0] + b[1] * 256 + h[0] * 65536)))
                pb.add_constraint((1 - pad) * (a[2] + a[3] * 256 + c[2] + c[3] * 256 + h[0] - (b[2] + b[3] * 256 + h[1] * 65536)))
        rel = pb.relation(z, alpha, 4)
        pb.add_to_relation(rel, 1 - pad, clk_next + pc_next)
        pb.finalize_logup(n_cols, shifts[1 + i])
        out.append(pb)
    bd = ap.ProgramBuilder()
    init_mult, final_mult, ipc0, ipc1, clk0, clk1, fpc0, fpc1 = [bd.next_trace_mask(k)[0] for k in range(8)]
    rel = bd.relation(z, alpha, 4)
    bd.add_to_relation(rel, init_mult, [clk0, clk1, ipc0, ipc1])
    bd.add_to_relation(rel, final_mult, [clk0, clk1, fpc0, fpc1])
    bd.finalize_logup(8, shifts[4])
    out.append(bd)
    return out


FIRST_SUM = 2        # index of an execution component's first sum constraint


def _statement(be, nz, mislabel=False, tamper=False):
    import nexus_zkvm_amd.air_program as ap
    cfg = nz.default_config(pow_bits=2)
    ex = _execution(mislabel)
    cls, src = ex["cls"], ex["src"]
    # the step table crosses to the device once, as words
    d_cls, d_src = _words(be, nz, cls), [_words(be, nz, s) for s in src]
    counts, part = be.trace_partition(d_cls.ptr.value, N_EXEC, 3)
    assert counts.sum() == N_EXEC and counts.all()
    log_cpu, logs, log_bd = nz.partition_log_size(N_EXEC, MIN_LOG), [nz.partition_log_size(int(c), MIN_LOG) for c in counts], MIN_LOG
    n_main = [4, EXEC_COLS, EXEC_COLS, NOP_COLS, 4]
    comp_logs = [log_cpu] + logs + [log_bd]
    tree_logs = [[log_cpu] * 2 + [log_bd] * 4, sum(([lg] * n for lg, n in zip(comp_logs, n_main)), []), sum(([lg] * k for lg, k in zip(comp_logs, [4, 4, 4, 4, 8])), [])]
    # preprocessed: the cpu component's clock (row + 1) and the boundary's multiplicities and initial pc
    row = np.arange(1 << log_cpu) + 1
    bd_pre = np.zeros((4, 1 << log_bd), np.uint32)
    bd_pre[0, 0], bd_pre[1, 1], bd_pre[2, 0], bd_pre[3, 0] = 1, P - 1, PC0 & 0xFFFF, PC0 >> 16
    pre_host = [M.to_storage(row & 0xFFFF, log_cpu).astype(np.uint32), M.to_storage(row >> 16, log_cpu).astype(np.uint32)] + [M.to_storage(r, log_bd) for r in bd_pre]
    s = be.prover_session(cfg, max(comp_logs))
    s.mix_u64(71)
    roots = [s.commit(pre_host)]
    pre_dev = [be.columns_from_host(c) for c in pre_host]
    main = s.tree_begin(tree_logs[1])
    at = np.concatenate([[0], np.cumsum(n_main)])
    comp_main = [main[at[i]:at[i + 1]] for i in range(5)]
    # one fill straight into the tree's columns: the cpu component from all steps, the three execution components from their classes
    dests = [{"cls": nz.PART_ALL, "log_size": log_cpu, "cols": comp_main[0][1:4], "limbs": [(S_PC, 2, 6), (S_PC, 8, 8), (S_PC, 16, 16)], "is_pad": comp_main[0][0]}]
    for i, kind in enumerate(KIND):
        lm = _exec_limbs(kind, aval_from_table=mislabel)
        dests.append({"cls": i, "log_size": logs[i], "cols": [comp_main[1 + i][k] for k in sorted(lm)], "limbs": [lm[k] for k in sorted(lm)],
                      "is_pad": comp_main[1 + i][6 if kind == "nop" else PAD]})
    part.fill([d.ptr.value for d in d_src], dests)
    part.destroy()
    for i, kind in enumerate(KIND):
        be.trace_program(_derive_program(ap, kind, aval_from_table=mislabel), comp_main[1 + i], logs[i])
    # the boundary: first (clk, pc) on row 0, last (clk-next, pc-next) on row 1
    bd_main = np.zeros((4, 1 << log_bd), np.uint32)
    final_pc = PC0 + 4 * N_EXEC
    bd_main[0, 0], bd_main[0, 1], bd_main[1, 1], bd_main[2, 1], bd_main[3, 1] = 1, (N_EXEC + 1) & 0xFFFF, (N_EXEC + 1) >> 16, final_pc & 0xFFFF, final_pc >> 16
    bd_host = [M.to_storage(r, log_bd) for r in bd_main]
    for d, col in zip(comp_main[4], bd_host):
        _upload(be, d, col)
    if tamper:                                                          # one pc limb of a real add row, after the fill
        col = nz.DeviceColumns.view(be, comp_main[1][PC], 1, logs[0]).to_cpu().reshape(-1)
        pad = nz.DeviceColumns.view(be, comp_main[1][PAD], 1, logs[0]).to_cpu().reshape(-1)
        pos = int(np.flatnonzero(pad == 0)[3])
        col[pos] = (int(col[pos]) + 4) % P
        _upload(be, comp_main[1][PC], col)
    got_main = [nz.DeviceColumns.view(be, d, 1, lg).to_cpu().reshape(-1) for d, lg in zip(main, tree_logs[1])]
    kept = [be.clone_columns(nz.DeviceColumns.view(be, d, 1, lg)) for d, lg in zip(main, tree_logs[1])]      # the commit turns columns into coefficients
    roots.append(s.tree_commit())
    z, alpha = s.draw_felt(), s.draw_felt()
    fracs = [p.build_logup() for p in _programs(ap, z, alpha, [(0, 0, 0, 0)] * 5)]
    inter = s.tree_begin(tree_logs[2])
    iat = np.concatenate([[0], np.cumsum([4, 4, 4, 4, 8])])
    kp = lambda i: [k.ptr.value for k in kept[at[i]:at[i + 1]]]
    ins = [[pre_dev[0].ptr.value, pre_dev[1].ptr.value] + kp(0), kp(1), kp(2), kp(3), [p.ptr.value for p in pre_dev[2:]] + kp(4)]
    claimed, shifts = [], []
    for i, (frac, cols, log) in enumerate(zip(fracs, ins, comp_logs)):
        out = inter[iat[i]:iat[i + 1]]
        assert 4 * frac.n_logup_cols == len(out)
        be.logup_program(frac, cols + [None] * len(out), log, out_ptrs=out)
        claimed.append(be.logup_finalize_last(out[-4:], log_size=log))
        n_inv = pow((1 << log) % P, P - 2, P)
        shifts.append([(int(x) * n_inv) % P for x in claimed[-1]])
    claimed = np.array(claimed, np.uint32)
    if tamper:
        s.close()
        return {"claimed": claimed}
    s.mix_felts(claimed)
    roots.append(s.tree_commit())
    progs = _programs(ap, z, alpha, shifts)
    mains = lambda i: [(1, int(k)) for k in range(at[i], at[i + 1])]
    inters = lambda i: [(2, int(k)) for k in range(iat[i], iat[i + 1])]
    comps = [ap.Component(log_cpu, progs[0].build(), [(0, 0), (0, 1)] + mains(0) + inters(0))]
    comps += [ap.Component(logs[i], progs[1 + i].build(), mains(1 + i) + inters(1 + i)) for i in range(3)]
    comps.append(ap.Component(log_bd, progs[4].build(), [(0, 2 + k) for k in range(4)] + mains(4) + inters(4)))
    return {"claimed": claimed, "session": s, "cfg": cfg, "comps": comps, "roots": roots, "z": z, "alpha": alpha, "tree_logs": tree_logs, "pre_host": pre_host,
            "bd_host": bd_host, "got_main": got_main, "ex": ex, "counts": counts, "logs": logs, "log_cpu": log_cpu, "at": at}


def _model_main_columns(st):
    """every main column from the model and host arithmetic: what a host without the two calls would build and upload"""
    ex, cols = st["ex"], []
    steps_of = M.partition(ex["cls"], 3)[1]
    r = M.fill(ex["cls"], 3, ex["src"], {"cls": M.ALL, "log_size": st["log_cpu"], "limbs": [(S_PC, 2, 6), (S_PC, 8, 8), (S_PC, 16, 16)]})
    cols += [r["is_pad"]] + r["cols"]
    for i, kind in enumerate(KIND):
        lm = _exec_limbs(kind, aval_from_table=False)
        r = M.fill(ex["cls"], 3, ex["src"], {"cls": i, "log_size": st["logs"][i], "limbs": [lm[k] for k in sorted(lm)]}, steps_of)
        c = dict(zip(sorted(lm), r["cols"]))
        c[6 if kind == "nop" else PAD] = r["is_pad"]
        _host_derived(kind, c)
        cols += [c[k] for k in range(NOP_COLS if kind == "nop" else EXEC_COLS)]
    return cols + st["bd_host"]


def _sums(claimed):
    return [int(sum(int(c[q]) for c in claimed) % P) for q in range(4)]


def test_a_v2_shaped_statement_from_a_step_table_is_proved_and_verified(be, nz):
    st = _statement(be, nz)
    s, comps, roots, tree_logs = st["session"], st["comps"], st["roots"], st["tree_logs"]
    # the claimed sums cancel only if every step sits in exactly one execution component, in a row of its own
    assert _sums(st["claimed"]) == [0, 0, 0, 0]
    assert all(c.any() for c in st["claimed"])
    want_main = _model_main_columns(st)
    for k, (g, w) in enumerate(zip(st["got_main"], want_main)):
        assert np.array_equal(g, w), "main column %d" % k
    carries = [int(st["got_main"][st["at"][1 + i] + (5 if kind == "nop" else PC_CARRY)].sum()) for i, kind in enumerate(KIND)]
    assert sum(carries) == 1                                           # the 16-bit boundary of pc is crossed once
    report = s.check(comps)
    assert report.ok, report
    words = s.prove(comps)
    v = nz.VerifierSession(st["cfg"])
    v.mix_u64(71)
    v.commit(roots[0], tree_logs[0])
    v.commit(roots[1], tree_logs[1])
    assert np.array_equal(v.draw_felt(), st["z"]) and np.array_equal(v.draw_felt(), st["alpha"])
    v.mix_felts(st["claimed"])
    v.commit(roots[2], tree_logs[2])
    assert v.verify(comps, words) is None
    assert np.array_equal(v.digest(), s.digest())
    s.close()
    # the same main tree from a session fed the model's columns by the host: byte-equal root
    h = be.prover_session(st["cfg"], max(tree_logs[1]))
    h.mix_u64(71)
    assert np.array_equal(h.commit(st["pre_host"]), roots[0])
    for d, col in zip(h.tree_begin(tree_logs[1]), want_main):
        _upload(be, d, col)
    assert np.array_equal(h.tree_commit(), roots[1])
    h.close()


def test_a_step_labelled_with_another_opcode_is_named_by_the_check(be, nz):
    """one ADD step labelled SUB before create, AVal taken from the execution's result: the sums still cancel (the step is in exactly
    one component), the check names the sub component, its first sum constraint and the step's ordinal among the SUB steps"""
    st = _statement(be, nz, mislabel=True)
    ex = st["ex"]
    assert _sums(st["claimed"]) == [0, 0, 0, 0]
    report = st["session"].check(st["comps"])
    st["session"].close()
    ordinal = int((ex["cls"][:ex["victim"]] == SUB).sum())
    assert not report.ok and report.n_failed in (1, 2)
    first = report.failures[0]
    assert (first.component, first.constraint, first.first_row, first.n_rows) == (2, FIRST_SUM, ordinal, 1), report
    assert all(f.component == 2 and f.first_row == ordinal for f in report.failures)


def test_a_pc_limb_changed_after_the_fill_unbalances_the_sums(be, nz):
    off = _statement(be, nz, tamper=True)
    assert _sums(off["claimed"]) != [0, 0, 0, 0]
