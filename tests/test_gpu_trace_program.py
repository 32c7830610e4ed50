"""nx_trace_program on the device: derived trace columns filled where the trace lives.  Every word is compared with the numpy
interpreter of tests/trace_programs.py (natural-row semantics, every operation reduced at once, mapped to the stored order with the
permutation of test_trace_check_cpu.py); the closed loop also against a second session that uploads the WHOLE trace computed by plain
numpy formulas: the same root, the same proof bytes."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import oracle_lib as O
import trace_programs as TP
from test_trace_check_cpu import natural_row_of_pos
from test_trace_program_cpu import GOOD, NX_ERR_ARG, refusal_cases

pytestmark = pytest.mark.gpu
P = O.P


@pytest.fixture(scope="module")
def be():
    import nexus_zkvm_amd as nz
    b = nz.HipBackend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def ap():
    import nexus_zkvm_amd.air_program as ap
    return ap


FILL = 0xDEADBEEF           # not a field element: a store that is missing shows


def run(be, prog, n_cols, inputs_nat, log_size, shift_words=0):
    """Uploads the inputs (the other columns hold FILL), runs the program, returns (device columns, interpreter's columns), stored order.
    shift_words: the columns start that many words into their allocation (1: no column is 16-byte aligned)."""
    n = 1 << log_size
    nat = [np.asarray(c, np.uint64) for c in inputs_nat] + [np.full(n, FILL, np.uint64) for _ in range(n_cols - len(inputs_nat))]
    host = np.full((n_cols + 1) * n, FILL, np.uint32)
    host[shift_words:shift_words + n_cols * n] = np.stack([TP.to_storage(c) for c in nat]).astype(np.uint32).reshape(-1)
    d = be.columns_from_host(host.reshape(n_cols + 1, n))
    be.trace_program(prog, [d.ptr.value + 4 * shift_words + k * (4 << log_size) for k in range(n_cols)], log_size)
    back = d.to_cpu().reshape(-1)
    assert np.all(back[:shift_words] == FILL) and np.all(back[shift_words + n_cols * n:] == FILL)          # nothing beyond the columns
    got = back[shift_words:shift_words + n_cols * n].reshape(n_cols, n)
    want = np.stack([TP.to_storage(c) for c in TP.interp(prog, nat, log_size)]).astype(np.uint32)
    return got, want


def pos_of_row(log, row):
    return int(np.nonzero(natural_row_of_pos(log) == row)[0][0])


# ---------------------------------------------------------------- the opcode table ----------
@pytest.mark.parametrize("log_size", [5, 6, 8, 11])
def test_opcode_table(be, log_size):
    """half a wave, one wave, one block, several blocks: every new opcode on all ordered pairs of EDGE, bit-exact"""
    prog, n_cols, _ = TP.opcode_table()
    got, want = run(be, prog, n_cols, TP.opcode_table_inputs(log_size), log_size)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert int(got[2:].max()) < P


# ---------------------------------------------------------------- offsets and the row ----------
@pytest.mark.parametrize("log_size", [5, 11])
def test_offsets_and_row(be, log_size):
    prog, n_cols, _ = TP.offsets_program()
    n = 1 << log_size
    a = np.random.default_rng(log_size).integers(0, P, n).astype(np.uint64)
    got, want = run(be, prog, n_cols, [a], log_size)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # the rows where an offset leaves one half of the circle domain or wraps, by name (column 1 + k holds a[i + OFFSETS[k]], 5 the row)
    for row in (0, 1, n - 2, n - 1):
        pos = pos_of_row(log_size, row)
        assert int(got[5][pos]) == row
        for k, o in enumerate(TP.OFFSETS):
            assert int(got[1 + k][pos]) == int(a[(row + o) % n]), (row, o)


# ---------------------------------------------------------------- STORE_IF ----------
def test_store_if_shares_a_column_and_keeps_the_rest(be):
    prog, n_cols, _ = TP.store_if_program()
    log_size = 8
    inputs = TP.store_if_inputs(log_size)
    got, want = run(be, prog, n_cols, inputs, log_size)
    assert np.array_equal(got, want)
    shared = got[5][np.argsort(natural_row_of_pos(log_size))]            # natural order
    assert np.all(shared[3::4] == TP.SENTINEL) and not np.any(shared[0::4] == TP.SENTINEL)      # the fourth flag wrote nothing
    again, _ = run(be, prog, n_cols, inputs, log_size)
    assert np.array_equal(again, got)


@pytest.mark.parametrize("log_size,shift_words", [(1, 0), (8, 1)])
def test_small_and_unaligned_traces(be, log_size, shift_words):
    """two rows, and columns that are not 16-byte aligned: the four-positions-per-lane kernel does not apply, the words are the same"""
    prog, n_cols, _ = TP.store_if_program()
    got, want = run(be, prog, n_cols, TP.store_if_inputs(log_size), log_size, shift_words)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- segments ----------
@pytest.mark.parametrize("vec4", [1, 0])
def test_segmented_program_gives_the_same_columns_in_both_kernel_shapes(be, vec4):
    """"air.segment" at 200 and at the default; "trace.vec4": four storage positions per lane (the default) and one row per lane"""
    prog, n_cols, _ = TP.opcode_table()
    assert int((np.asarray(prog.instrs)[:, 0] == 32).sum()) >= 40
    default = be.get_option("air.segment")
    assert be.get_option("trace.vec4") == 1
    try:
        be.set_option("trace.vec4", vec4)
        be.set_option("air.segment", 200)
        cut, want = run(be, prog, n_cols, TP.opcode_table_inputs(8), 8)
        be.set_option("air.segment", default)
        whole, _ = run(be, prog, n_cols, TP.opcode_table_inputs(8), 8)
    finally:
        be.set_option("air.segment", default)
        be.set_option("trace.vec4", 1)
    assert np.array_equal(cut, whole) and np.array_equal(cut, want)


# ---------------------------------------------------------------- preprocessed columns ----------
def test_is_first_and_a_row_counter(be, ap):
    pb = ap.ProgramBuilder()
    pb.store(0, pb.eq(pb.row(), 0))
    pb.store(1, pb.row())
    prog = pb.build_trace_program()
    got, want = run(be, prog, 2, [], 6)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], TP.to_storage((np.arange(64) == 0).astype(np.uint32)))
    assert np.array_equal(got[1], TP.to_storage(np.arange(64, dtype=np.uint32)))


# ---------------------------------------------------------------- the closed loop ----------
LOG = 8
# the main tree: 12 seed columns (bytes), 27 derived ones
B, Cc, SH, F_ADD, F_SLL, F_XOR = 0, 4, 8, 9, 10, 11
VA, CARRY, S, H1, E, REM, QT, AND, INV_Z, IS_ZERO = 12, 16, 18, 23, 24, 25, 29, 33, 37, 38
N_MAIN, N_SEED = 39, 12


def seeds():
    """natural order: two 4-byte operands, a shift amount (0 on some rows), three disjoint opcode flags (row i belongs to chip i % 3)"""
    rng = np.random.default_rng(2024)
    n = 1 << LOG
    b = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(4)]
    c = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(4)]
    for k in range(4):
        b[k][:3], c[k][:3] = 255, 255                 # every carry set, in each chip's first row
    sh = rng.integers(0, 32, n, dtype=np.uint8)
    sh[::5] = 0
    flags = [(np.arange(n) % 3 == k).astype(np.uint8) for k in range(3)]
    return b + c + [sh] + flags


def whole_trace(seed):
    """The 39 main columns in natural order by plain numpy formulas (what a host would have computed and uploaded)."""
    t = [np.asarray(s, np.uint64) for s in seed] + [None] * (N_MAIN - N_SEED)
    b, c, sh = t[B:B + 4], t[Cc:Cc + 4], t[SH]
    lo = b[0] + c[0] + 256 * (b[1] + c[1])
    hi = b[2] + c[2] + 256 * (b[3] + c[3]) + (lo >> 16)
    add = [lo & 255, (lo >> 8) & 255, hi & 255, (hi >> 8) & 255]
    t[CARRY], t[CARRY + 1] = lo >> 16, hi >> 16
    for k in range(5):
        t[S + k] = (sh >> k) & 1
    t[H1] = (1 + t[S]) * (1 + 3 * t[S + 1])
    t[E] = np.uint64(1) << (sh & 7)
    assert np.array_equal(t[E], t[H1] * (1 + 15 * t[S + 2]))
    for k in range(4):
        t[REM + k], t[QT + k] = (b[k] * t[E]) & 255, (b[k] * t[E]) >> 8
        t[AND + k] = b[k] & c[k]
    sll = [t[REM + k] + (t[QT + k - 1] if k else 0) for k in range(4)]
    xor = [b[k] ^ c[k] for k in range(4)]
    for k in range(4):
        t[VA + k] = np.where(t[F_ADD] == 1, add[k], np.where(t[F_SLL] == 1, sll[k], xor[k]))
    t[INV_Z] = np.array([pow(int(v), P - 2, P) for v in sh], np.uint64)
    t[IS_ZERO] = (sh == 0).astype(np.uint64)
    return [np.asarray(x, np.uint64) for x in t]


def derivation(ap):
    """fill_main_trace's row-local part, in the test's own words"""
    pb = ap.ProgramBuilder()
    col = lambda k: pb.next_trace_mask(k)[0]
    b, c, sh = [col(B + k) for k in range(4)], [col(Cc + k) for k in range(4)], col(SH)
    f_add, f_sll, f_xor = col(F_ADD), col(F_SLL), col(F_XOR)
    # AddChip: byte limbs, carries at the 16-bit boundaries
    lo = b[0] + c[0] + (b[1] + c[1]) * 256
    carry0 = pb.shr(lo, 16)
    hi = b[2] + c[2] + (b[3] + c[3]) * 256 + carry0
    pb.store(CARRY, carry0)
    pb.store(CARRY + 1, pb.shr(hi, 16))
    for k, v in enumerate((pb.band(lo, 255), pb.band(pb.shr(lo, 8), 255), pb.band(hi, 255), pb.band(pb.shr(hi, 8), 255))):
        pb.store_if(f_add, VA + k, v)
    # SllChip: shift bits, Helper1, Exp1_3 = 2^(sh & 7), remainder and quotient limbs
    bits = [pb.band(pb.shr(sh, k), 1) for k in range(5)]
    for k in range(5):
        pb.store(S + k, bits[k])
    pb.store(H1, pb.shl(1, pb.band(sh, 3)))
    e = pb.shl(1, pb.band(sh, 7))
    pb.store(E, e)
    rem, qt = [pb.band(b[k] * e, 255) for k in range(4)], [pb.shr(b[k] * e, 8) for k in range(4)]
    for k in range(4):
        pb.store(REM + k, rem[k])
        pb.store(QT + k, qt[k])
        pb.store_if(f_sll, VA + k, rem[k] + qt[k - 1] if k else rem[k])
    # the bitwise chip: XOR result, AND helper
    for k in range(4):
        pb.store(AND + k, pb.band(b[k], c[k]))
        pb.store_if(f_xor, VA + k, pb.bxor(b[k], c[k]))
    # is-zero of the shift amount through the inverse
    inv = pb.inv(sh)
    pb.store(INV_Z, inv)
    pb.store(IS_ZERO, 1 - sh * inv)
    return pb.build_trace_program()


ADD_LOW = 0         # the ordinal of the add chip's low-limb constraint


def constraints(ap):
    pb = ap.ProgramBuilder()
    t = [pb.next_trace_mask(k)[0] for k in range(N_MAIN)]
    b, c, sh, va = t[B:B + 4], t[Cc:Cc + 4], t[SH], t[VA:VA + 4]
    pb.add_constraint(t[F_ADD] * (b[0] + c[0] + (b[1] + c[1]) * 256 - va[0] - va[1] * 256 - t[CARRY] * 65536))                  # ADD_LOW
    pb.add_constraint(t[F_ADD] * (b[2] + c[2] + (b[3] + c[3]) * 256 + t[CARRY] - va[2] - va[3] * 256 - t[CARRY + 1] * 65536))
    for k in range(2):
        pb.add_constraint(t[CARRY + k] * (t[CARRY + k] - 1))
    pb.add_constraint(sh - t[S] - t[S + 1] * 2 - t[S + 2] * 4 - t[S + 3] * 8 - t[S + 4] * 16)
    for k in range(5):
        pb.add_constraint(t[S + k] * (t[S + k] - 1))
    pb.add_constraint(t[H1] - (t[S] + 1) * (t[S + 1] * 3 + 1))
    pb.add_constraint(t[E] - t[H1] * (t[S + 2] * 15 + 1))
    for k in range(4):
        pb.add_constraint(b[k] * t[E] - t[QT + k] * 256 - t[REM + k])
    for k in range(4):
        pb.add_constraint(t[F_SLL] * (va[k] - t[REM + k] - (t[QT + k - 1] if k else 0)))
    for k in range(4):
        pb.add_constraint(t[F_XOR] * (va[k] - b[k] - c[k] + t[AND + k] * 2))
    pb.add_constraint(sh * t[INV_Z] - 1 + t[IS_ZERO])
    pb.add_constraint(t[IS_ZERO] * sh)
    pb.add_constraint(t[F_ADD] + t[F_SLL] + t[F_XOR] - 1)
    return ap.Component(LOG, pb.build(), [(0, k) for k in range(N_MAIN)])


def derived_session(be, nz, ap, cfg, seed, tamper=None):
    """A session whose main tree holds the seeds (narrow upload) and what nx_trace_program derives from them.  tamper: (column, natural
    row, value) written into a SEED column after the derivation.  Returns (session, the tree's columns before the commit, root)."""
    s = be.prover_session(cfg, LOG)
    ptrs = s.tree_begin([LOG] * N_MAIN)
    arrs, kinds = nz._narrow_columns(seed)
    assert list(kinds) == [nz.COL_U8] * N_SEED
    table = (C.c_void_p * N_SEED)(*ptrs[:N_SEED])
    be._chk(be.L.nx_upload_columns_narrow(be.ctx, *nz._host_columns(arrs, kinds), N_SEED, LOG, table, 1))
    be.trace_program(derivation(ap), ptrs, LOG)
    if tamper:
        k, row, value = tamper
        word = np.array([value], np.uint32)
        be._chk(be.L.nx_upload(be.ctx, C.c_void_p(ptrs[k] + 4 * pos_of_row(LOG, row)), word.ctypes.data_as(C.c_void_p), C.c_size_t(1)))
    cols = np.stack([nz.DeviceColumns.view(be, p, 1, LOG).to_cpu().reshape(-1) for p in ptrs])
    return s, cols, s.tree_commit()


def test_closed_loop_derive_check_prove_verify(be, nz, ap, oracle):
    ocfg = O.default_cfg(pow_bits=2)
    cfg = nz.PcsConfig(*[int(x) for x in ocfg])
    seed = seeds()
    trace = whole_trace(seed)
    # the two references agree: plain numpy formulas and the interpreter running the recorded derivation
    by_interp = TP.interp(derivation(ap), [np.asarray(x, np.uint64) for x in seed] + [np.full(1 << LOG, FILL, np.uint64)] * (N_MAIN - N_SEED), LOG)
    assert all(np.array_equal(x, y) for x, y in zip(by_interp, trace))
    assert trace[CARRY].any() and trace[CARRY + 1].any() and trace[IS_ZERO].any() and not trace[IS_ZERO].all() and int(trace[E].max()) == 128
    stored = np.stack([TP.to_storage(x) for x in trace]).astype(np.uint32)
    comp = constraints(ap)
    # 1. the device fills the derived columns
    s, cols, root = derived_session(be, nz, ap, cfg, seed)
    assert np.array_equal(cols, stored), np.argwhere(cols != stored)[:8]
    # 2. the recorded constraints hold on them
    rep = s.check([comp])
    assert rep.ok, rep
    words = s.prove([comp])
    # 3. a session that uploads the whole trace: the same root, the same proof
    s2 = be.prover_session(cfg, LOG)
    assert np.array_equal(s2.commit(list(stored)), root)
    assert np.array_equal(s2.prove([comp]), words)
    # 4. the verifiers accept
    for v in (nz.VerifierSession(cfg), O.VerifierSession(ocfg)):
        v.commit(root, [LOG] * N_MAIN)
        assert v.verify([comp], words) is None
    s.close(); s2.close()
    # 5. one seed byte changed after the derivation: the add constraint, that row, nothing else
    row = 9                                                 # 9 % 3 == 0: an add row
    s3, _, _ = derived_session(be, nz, ap, cfg, seed, tamper=(Cc, row, (int(seed[Cc][row]) + 1) % 256))
    rep = s3.check([comp])
    assert not rep.ok and [(f.component, f.constraint, f.first_row, f.n_rows) for f in rep.failures] == [(0, ADD_LOW, row, 1)]
    assert rep.message.endswith(f"component 0 constraint {ADD_LOW}: not zero on 1 of {1 << LOG} rows, first at row {row}")
    s3.close()


# ---------------------------------------------------------------- refusals and reuse ----------
def test_refusals_leave_the_context_usable_and_nothing_allocated(be):
    log_size = 5
    d = be.columns_from_host(np.stack([np.arange(32), np.full(32, FILL), np.full(32, FILL), np.full(32, FILL)]).astype(np.uint32))
    real = [d.ptr.value + k * (4 << log_size) for k in range(4)]
    fake = {None: None, 0x1000: real[0], 0x2000: real[1]}
    f = be.L.nx_trace_program
    be.sync()
    live0, _ = be.memory(reset_peak=True)
    for name, instrs, n_regs, n_cols, ptrs, lg, named in refusal_cases():
        ins = np.ascontiguousarray(np.asarray(instrs, dtype=np.int64).astype(np.uint32).reshape(-1))
        table = (C.c_void_p * n_cols)(*([fake[p] for p in ptrs] if ptrs is not None else real[:n_cols]))
        rc = f(be.ctx, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, n_regs, table, n_cols, lg, None)
        msg = be.L.nx_last_error(be.ctx).decode()
        assert rc == NX_ERR_ARG, (name, rc, msg)
        if named is not None:
            assert f"instruction {named}:" in msg, (name, msg)
    assert f(be.ctx, None, 0, 2, (C.c_void_p * 2)(*real[:2]), 2, log_size, None) == NX_ERR_ARG
    ins = np.asarray(GOOD, np.uint32).reshape(-1)
    assert f(be.ctx, ins.ctypes.data_as(C.c_void_p), 4, 2, None, 2, log_size, None) == NX_ERR_ARG             # no column table
    # the context then runs a valid program (column 1 = column 0 ^ 5), and holds what it held
    assert f(be.ctx, ins.ctypes.data_as(C.c_void_p), 4, 2, (C.c_void_p * 2)(*real[:2]), 2, log_size, None) == 0
    got = d.to_cpu()
    live1, _ = be.memory()
    assert live1 == live0
    assert np.array_equal(got[0], np.arange(32)) and np.array_equal(got[1], np.arange(32) ^ 5) and np.all(got[2:] == FILL)
