"""The 32-bit integer register kind of nx_trace_program and the RV32M chips on the device.  The opcode table against the interpreter of
tests/rv32m_model.py on all ordered pairs of E; the five chips' columns from ValueB, ValueC and the opcode flags in ONE nx_trace_program
call against the model, word for word, for each of the eight opcodes; the closed loop: seeds uploaded, the fill into tree_begin's
columns, multiplicities counted on the device, the statement checked, balanced, proved and verified, with the main root of a session
fed the model's columns from the host."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import oracle_lib as O
import rv32m_air as A
import rv32m_model as M
import trace_programs as TP
from test_gpu_trace_program import FILL, pos_of_row
from test_rv32m_cpu import refusal_cases
from test_trace_program_cpu import NX_ERR_ARG

pytestmark = pytest.mark.gpu
P = O.P
LOG = M.LOG
NX_ERR_PROTOCOL = -4


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


def run(be, prog, before_nat, log_size, shift_words=0):
    """Uploads the columns (natural order given), runs the program, returns the device columns in the stored order.  shift_words: the
    columns start that many words into their allocation (1: no column is 16-byte aligned, the word path runs)."""
    n, n_cols = 1 << log_size, len(before_nat)
    host = np.full((n_cols + 1) * n, FILL, np.uint32)
    host[shift_words:shift_words + n_cols * n] = np.stack([TP.to_storage(c) for c in before_nat]).astype(np.uint32).reshape(-1)
    d = be.columns_from_host(host.reshape(n_cols + 1, n))
    be.trace_program(prog, [d.ptr.value + 4 * shift_words + k * (4 << log_size) for k in range(n_cols)], log_size)
    back = d.to_cpu().reshape(-1)
    assert np.all(back[:shift_words] == FILL) and np.all(back[shift_words + n_cols * n:] == FILL)          # nothing beyond the columns
    return back[shift_words:shift_words + n_cols * n].reshape(n_cols, n)


def stored(cols_nat):
    return np.stack([TP.to_storage(c) for c in cols_nat]).astype(np.uint32)


# ---------------------------------------------------------------- the opcode table ----------
@pytest.fixture(scope="module")
def table():
    """(program, {log size: (inputs, the interpreter's columns)}) — computed once"""
    prog = A.opcode_table()
    want = {}
    for lg in (1, 2, 6, 9):
        before = A.opcode_table_inputs(lg) + [np.full(1 << lg, FILL, np.uint64)] * (A.TABLE_COLS - A.TABLE_INPUTS)
        want[lg] = (before, stored(M.interp(prog, before, lg)))
    return prog, want


@pytest.mark.parametrize("vec4", [1, 0])
@pytest.mark.parametrize("log_size", [1, 2, 6, 9])
def test_opcode_table(be, table, log_size, vec4):
    """two rows, one lane of four, one wave, two blocks; all 441 ordered pairs of E at 2^9: a zero divisor, divisors of 2^31 and above,
    both sides of the float mantissa the reciprocal goes through, products that fill 64 bits"""
    prog, want = table
    try:
        be.set_option("trace.vec4", vec4)
        got = run(be, prog, want[log_size][0], log_size)
    finally:
        be.set_option("trace.vec4", 1)
    assert np.array_equal(got, want[log_size][1]), np.argwhere(got != want[log_size][1])[:8]
    assert int(got.max()) < 1 << 16


def test_opcode_table_on_columns_shifted_by_one_word(be, table):
    prog, want = table
    got = run(be, prog, want[9][0], 9, shift_words=1)
    assert np.array_equal(got, want[9][1]), np.argwhere(got != want[9][1])[:8]


# ---------------------------------------------------------------- the five chips ----------
@pytest.fixture(scope="module")
def fill():
    return A.fill_program()


@pytest.mark.parametrize("op", M.OPS)
def test_fill_equals_the_model_word_for_word(be, fill, op):
    """441 rows of `op`, 71 rows of other opcodes whose ValueA holds a sentinel"""
    ops, operands = M.trace_ops(op)
    before, after = M.seeds_and_trace(ops, operands)
    got, want = run(be, fill, before, LOG), stored(after)
    assert np.array_equal(got, want), [(k, int(r)) for k, r in np.argwhere(got != want)[:8]]
    idle = TP.to_storage(np.array([o is None for o in ops]))
    for k in M.cols_of("ValueA"):
        assert np.all(got[k][idle] == M.SENTINEL) and not np.any(got[k][~idle] == M.SENTINEL)


@pytest.mark.parametrize("vec4", [1, 0])
def test_segmented_fill_gives_the_same_columns(be, fill, vec4):
    """"air.segment" at its smallest: a kernel per store, the division recomputed in every kernel that stores a Quotient byte"""
    ops, operands = M.trace_ops("rem")
    before, after = M.seeds_and_trace(ops, operands)
    default = be.get_option("air.segment")
    try:
        be.set_option("trace.vec4", vec4)
        be.set_option("air.segment", 200)
        cut = run(be, fill, before, LOG)
    finally:
        be.set_option("air.segment", default)
        be.set_option("trace.vec4", 1)
    assert np.array_equal(cut, stored(after))


# ---------------------------------------------------------------- the closed loop ----------
BYTE_SENTINEL = 0xA5                      # ValueA is a byte column of the statement: the rows of other opcodes hold a byte
LOG_256, LOG_8 = 8, 3


def statement_rows():
    """every pair once, the opcodes in turn; the 71 other rows are rows of other opcodes"""
    ops = [M.OPS[i % 8] for i in range(len(M.PAIRS))] + [None] * ((1 << LOG) - len(M.PAIRS))
    return ops, M.PAIRS + [(0, 0)] * ((1 << LOG) - len(M.PAIRS))


@pytest.fixture(scope="module")
def statement():
    ops, operands = statement_rows()
    before, after = M.seeds_and_trace(ops, operands, sentinel=BYTE_SENTINEL)
    bytes_used = np.concatenate([after[k] for k in A.byte_lookup_columns()]).astype(np.int64)
    mult = [np.bincount(bytes_used, minlength=256).astype(np.uint32), np.bincount(after[M.COL["MulCarry1"]].astype(np.int64), minlength=8).astype(np.uint32)]
    return ops, before, after, mult


def components(z, alpha, shifts):
    """the chips' component and the two range tables; tree 0: the table values, tree 1: the main columns, tree 2: the interaction"""
    main = A.constraints(LOG, lookups=((z[0], z[1]), (alpha[0], alpha[1]), shifts[0], 0))
    main.log_constraint_degree_bound = 2                        # the v1 main component's bound: its DIV / REM constraints have degree 4
    n_inter = 4 * main.builder.n_logup_cols
    t256 = A.table(LOG_256, z[0], alpha[0], shifts[1], [(0, 0), (1, M.N_COLS)] + [(2, n_inter + k) for k in range(4)])
    t8 = A.table(LOG_8, z[1], alpha[1], shifts[2], [(0, 1), (1, M.N_COLS + 1)] + [(2, n_inter + 4 + k) for k in range(4)])
    return [main, t256, t8], n_inter


def upload_word(be, ptr, log_size, row, value):
    word = np.array([value], np.uint32)
    be._chk(be.L.nx_upload(be.ctx, C.c_void_p(ptr + 4 * pos_of_row(log_size, row)), word.ctypes.data_as(C.c_void_p), C.c_size_t(1)))


def session(be, nz, statement, tamper=None):
    """Seeds uploaded, ONE nx_trace_program into tree_begin's columns, multiplicities from nx_logup_multiplicities, the interaction trace.
    tamper: (column, natural row, value) written after the fill.  Returns a dict of what the tests look at."""
    ops, before, after, mult = statement
    ocfg = O.default_cfg(pow_bits=2, log_constraint_degree=2)
    cfg = nz.PcsConfig(*[int(x) for x in ocfg])
    values = [np.arange(1 << LOG_256, dtype=np.uint32), np.arange(1 << LOG_8, dtype=np.uint32)]     # value i at storage position i
    out = {"cfg": cfg, "ocfg": ocfg}
    s = out["s"] = be.prover_session(cfg, LOG)
    s.mix_u64(32)
    roots = out["roots"] = [s.commit(values)]
    tables = [be.columns_from_host(v) for v in values]
    main_logs = [LOG] * M.N_COLS + [LOG_256, LOG_8]
    main = s.tree_begin(main_logs)
    for k in list(range(M.N_SEED)) + M.cols_of("ValueA"):
        host = np.ascontiguousarray(TP.to_storage(before[k]), dtype=np.uint32)
        be._chk(be.L.nx_upload(be.ctx, C.c_void_p(main[k]), host.ctypes.data_as(C.c_void_p), C.c_size_t(len(host))))
    be.trace_program(A.fill_program(), main[:M.N_COLS], LOG)
    if tamper:
        upload_word(be, main[tamper[0]], LOG, tamper[1], tamper[2])
    res256 = be.logup_multiplicities([([main[k]], None, LOG) for k in A.byte_lookup_columns()], [tables[0].ptr.value], LOG_256, [8], main[M.N_COLS], want_rc=True)
    res8 = be.logup_multiplicities([([main[M.COL["MulCarry1"]]], None, LOG)], [tables[1].ptr.value], LOG_8, [3], main[M.N_COLS + 1], want_rc=True)
    out["missing"] = (res256, res8)
    kept = [be.clone_columns(nz.DeviceColumns.view(be, d, 1, lg)) for d, lg in zip(main, main_logs)]      # the commit turns columns into coefficients
    out["main"] = [k.to_cpu().reshape(-1) for k in kept]
    roots.append(s.tree_commit())
    z, alpha = [s.draw_felt(), s.draw_felt()], [s.draw_felt(), s.draw_felt()]
    out["elements"] = (z, alpha)
    comps, n_inter = components(z, alpha, [(0, 0, 0, 0)] * 3)
    inter_logs = out["inter_logs"] = [LOG] * n_inter + [LOG_256] * 4 + [LOG_8] * 4
    inter = s.tree_begin(inter_logs)
    ins = [[k.ptr.value for k in kept[:M.N_COLS]], [tables[0].ptr.value, kept[M.N_COLS].ptr.value], [tables[1].ptr.value, kept[M.N_COLS + 1].ptr.value]]
    outs, logs = [inter[:n_inter], inter[n_inter:n_inter + 4], inter[n_inter + 4:]], [LOG, LOG_256, LOG_8]
    claimed, shifts = [], []
    for comp, cols, o, lg in zip(comps, ins, outs, logs):
        frac = comp.builder.build_logup()
        assert 4 * frac.n_logup_cols == len(o)
        be.logup_program(frac, cols + [None] * len(o), lg, out_ptrs=o)
        claimed.append(be.logup_finalize_last(o[-4:], log_size=lg))
        n_inv = pow((1 << lg) % P, P - 2, P)
        shifts.append([(int(x) * n_inv) % P for x in claimed[-1]])
    out["claimed"] = np.array(claimed, np.uint32)
    s.mix_felts(out["claimed"])
    roots.append(s.tree_commit())
    out["comps"] = components(z, alpha, shifts)[0]
    out["main_logs"] = main_logs
    return out


def test_closed_loop_fill_count_check_prove_verify(be, nz, statement, oracle):
    """At the context's default options; then the same statement under "air.quarter_domain" 0, 1 and 2: the same proof words each time
    (the chips' degree-5 constraints stay on the component's own domain, only the degree-4 ones go to the quarter: DESIGN.md item 75)."""
    quarter = be.get_option("air.quarter_domain")
    assert quarter == 2
    words = _closed_loop(be, nz, statement)
    try:
        for q in (0, 1, 2):
            be.set_option("air.quarter_domain", q)
            r = session(be, nz, statement)
            try:
                again = r["s"].prove(r["comps"])
            finally:
                r["s"].close()
            assert np.array_equal(again, words), ("air.quarter_domain", q)
    finally:
        be.set_option("air.quarter_domain", quarter)


def _closed_loop(be, nz, statement):
    """returns the proof words"""
    ops, before, after, mult = statement
    r = session(be, nz, statement)
    s = r["s"]
    # the device's main tree is the model's, multiplicities included
    want = [TP.to_storage(c).astype(np.uint32) for c in after] + mult
    assert r["missing"] == (((0, 0, 0), 0), ((0, 0, 0), 0))
    for k, (g, w) in enumerate(zip(r["main"], want)):
        assert np.array_equal(g, w), (k, np.nonzero(g != w)[0][:8])
    assert int(mult[1][1:].sum()) > 0 and int(mult[0].sum()) == len(A.byte_lookup_columns()) << LOG
    # balanced: the three claimed sums cancel, none of them is zero
    total = [int(sum(int(c[q]) for c in r["claimed"]) % P) for q in range(4)]
    assert total == [0, 0, 0, 0] and all(c.any() for c in r["claimed"])
    report = s.check(r["comps"])
    assert report.ok, report
    words = s.prove(r["comps"])
    z, alpha = r["elements"]
    for v in (nz.VerifierSession(r["cfg"]), O.VerifierSession(r["ocfg"])):
        v.mix_u64(32)
        v.commit(r["roots"][0], [LOG_256, LOG_8])
        v.commit(r["roots"][1], r["main_logs"])
        for e in z + alpha:
            assert np.array_equal(v.draw_felt(), e)
        v.mix_felts(r["claimed"])
        v.commit(r["roots"][2], r["inter_logs"])
        assert v.verify(r["comps"], words) is None
        assert np.array_equal(v.digest(), s.digest())
    s.close()
    # a session fed the model's columns from the host: the same main root
    s2 = be.prover_session(r["cfg"], LOG)
    s2.mix_u64(32)
    assert np.array_equal(s2.commit([np.arange(256, dtype=np.uint32), np.arange(8, dtype=np.uint32)]), r["roots"][0])
    assert np.array_equal(s2.commit(want), r["roots"][1])
    s2.close()
    return words


def test_one_changed_helper_t_byte_is_named_by_the_check(be, nz, statement):
    ops = statement[0]
    for op, chip in (("divu", "DivuRemu"), ("rem", "DivRem")):
        row = next(i for i, o in enumerate(ops) if o == op and M.PAIRS[i][1] > 1)
        k = M.COL["HelperT"]
        r = session(be, nz, statement, tamper=(k, row, int(statement[2][k][row]) ^ 1))          # still a byte: the lookups stay sound
        main = r["comps"][0]
        report = r["s"].check(r["comps"])
        assert not report.ok and report.failures
        assert all(f.component == 0 and main.chips[f.constraint] == chip and f.first_row == row and f.n_rows == 1 for f in report.failures), report
        assert f"component 0 constraint {report.failures[0].constraint}: not zero on 1 of {1 << LOG} rows, first at row {row}" in report.message
        r["s"].close()


def test_a_mul_p1_byte_of_256_unbalances_the_sums(be, nz, statement):
    ops = statement[0]
    row = next(i for i, o in enumerate(ops) if o == "mul")
    r = session(be, nz, statement, tamper=(M.COL["MulP1"], row, 256))
    (res256, rc256), (res8, rc8) = r["missing"]
    use = A.byte_lookup_columns().index(M.COL["MulP1"])
    assert rc256 == NX_ERR_PROTOCOL and res256 == (1, use, pos_of_row(LOG, row)) and (res8, rc8) == ((0, 0, 0), 0)     # 256 is in no table row
    total = [int(sum(int(c[q]) for c in r["claimed"]) % P) for q in range(4)]
    assert total != [0, 0, 0, 0]
    r["s"].close()


# ---------------------------------------------------------------- refusals ----------
def test_refusals_leave_the_context_usable_and_nothing_allocated(be):
    log_size = 5
    d = be.columns_from_host(np.stack([np.arange(32), np.full(32, FILL)]).astype(np.uint32))
    real = [d.ptr.value + k * (4 << log_size) for k in range(2)]
    f = be.L.nx_trace_program
    be.sync()
    live0, _ = be.memory(reset_peak=True)
    for name, instrs, n_regs, n_cols, named, word in refusal_cases():
        ins = np.ascontiguousarray(np.asarray(instrs, dtype=np.int64).astype(np.uint32).reshape(-1))
        rc = f(be.ctx, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, n_regs, (C.c_void_p * n_cols)(*real[:n_cols]), n_cols, log_size, None)
        msg = be.L.nx_last_error(be.ctx).decode()
        assert rc == NX_ERR_ARG and f"instruction {named}:" in msg and word in msg, (name, rc, msg)
    # the context then runs a valid program: column 1 = the high half of (x + (x << 16)) / 3
    import nexus_zkvm_amd.air_program as ap
    pb = ap.ProgramBuilder()
    (x,) = pb.next_trace_mask(0)
    pb.store(1, pb.hi16(pb.divu32(pb.pack32(x, x), pb.pack32(3, 0))))
    be.trace_program(pb.build_trace_program(), real, log_size)
    got = d.to_cpu()
    live1, _ = be.memory()
    assert live1 == live0
    assert np.array_equal(got[0], np.arange(32)) and np.array_equal(got[1], (np.arange(32) * 0x10001 // 3) >> 16)
