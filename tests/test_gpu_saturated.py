"""Every lazily reduced field sum at saturated operands (-m gpu).

Since round 6 the secure-field arithmetic adds products of canonical M31 words as raw 64-bit integers and folds "at least every 4
products" (csrc/field.cuh: 4 (p-1)^2 + 2^33 + 2^31 < 2^64; five do not fit).  The rule is applied by hand at a dozen sites — field.cuh's
q_mul / q_norm_cm / q_conj_times(_add), their copies in the kernel text of air_jit.hip, the emitted constraint sum and the dot-product
peephole's lazy accumulators, the interpreter (constraints.hip), logup.hip's three tuple sums and pcs.hip's three 4-step loops — and
uniformly random operands cannot tell a fold period of 4 from 5.  These tests feed every site
    SAT    every word p-1, or
    EDGE   words from {0, 1, p-1, p-2}, where "enumerated" = every combination laid out over the rows,
and compare, array_equal and every word < p, with a reduce-after-every-operation reference: the oracle (oracle/fields.h reduces every
product) and, for the hand-written programs, tests/saturated_programs.py::interp.  Where one factor is derived by the library and
cannot be saturated (T_hi of eval_at_point, c_k of the quotients) the columns are SAT and there are enough independent 5-product
windows (each overflows with probability 1/120 under a period of 5) for a wrong period to show.  Zero denominators — promised to
"give 0 like m_inv(0) and not poison their group" — are pinned on the same footing.

Out of scope: synth_constraints_kernel (csrc/air.hip) takes both factors from the device-filled synthetic trace and the channel, so
neither can be set by a caller; it has no direct test here (tools/ab/patches/fold_period_5.patch changes its period too, for a
mutation run of the parity proofs).

Compiled programs are kept few, hiprtc being what costs the time: the chains and the guards share one JIT kernel, one check kernel
(with the runs) and one fraction kernel.

tests/test_air_text_host_cpu.py is the CPU twin for the generated text."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libnexus_hip.so, as in test_gpu_parity.py)

import oracle_lib as O
import saturated_programs as SP

pytestmark = pytest.mark.gpu
P = O.P
SAT4 = (P - 1,) * 4
LOG_SIZE, LOG_EVAL = 5, 6


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


def _ptrs(d):
    return [d.ptr.value + k * (4 << d.log_size) for k in range(d.n_cols)]


def _canonical(*arrays):
    return all(int(np.asarray(a).max()) < P for a in arrays)


# ================================================================ 1. hand-written AIR programs ================================
PROGRAMS = {"chains": SP.chains_program, "guards": SP.guards_program, "runs": SP.runs_program, "guards+runs": lambda: SP.guards_program(runs=True),
            "chains+guards": SP.all_program}


@pytest.fixture(scope="module")
def sat_case():
    """name -> (program, SAT columns, SAT alpha powers, {denom word: expected accumulator}): the reference once per module"""
    cache = {}

    def get(name):
        if name not in cache:
            asm = PROGRAMS[name]()
            prog = asm.program(SP.sat_econsts())
            assert prog.n_regs <= 160                  # the interpreter's register file
            prog.marks = asm.marks
            cols, pw = SP.sat_inputs(prog, 1 << LOG_EVAL)
            cons, _ = SP.interp(prog, cols)
            start = np.full((4, 1 << LOG_EVAL), P - 1, np.uint32)
            want = {}
            for d in (1, P - 1):
                den = np.full(1 << (LOG_EVAL - LOG_SIZE), d, np.uint32)
                want[d] = SP.accumulate(cons, pw, den, LOG_SIZE, start)
                assert np.array_equal(want[d], np.stack(O.eval_constraint_program(prog, list(cols), pw, den, LOG_SIZE, LOG_EVAL, acc4=list(start)))), "the two references disagree"
                assert _canonical(want[d])
            cache[name] = (prog, cols, pw, start, want)
        return cache[name]
    return get


def _run_eval(b, run, sat, name):
    prog, cols, pw, start, want = sat(name)
    d_cols = b.columns_from_host(cols)
    for d in (1, P - 1):
        acc = b.columns_from_host(start)
        run(prog, _ptrs(d_cols), pw, np.full(1 << (LOG_EVAL - LOG_SIZE), d, np.uint32), acc)
        got = acc.to_cpu()
        assert _canonical(got) and np.array_equal(got, want[d]), (name, d)


@pytest.mark.parametrize("name", ["chains", "guards", "runs"])
def test_interpreter_on_saturated_programs(be, oracle, sat_case, name):
    """constraints.hip: the `++pending == 4` of the constraint sum ("runs": 9 consecutive CONSTRAINT_B, CONSTRAINT_B / _E alternating),
    and the literal semantics the JIT's fused chains must reproduce ("chains", "guards")"""
    _run_eval(be, lambda prog, ptrs, pw, den, acc: be.eval_constraint_program(prog, ptrs, pw, den, LOG_SIZE, LOG_EVAL, acc), sat_case, name)


def test_jit_dot_chains_and_peephole_guards_on_saturated_operands(be, oracle, sat_case):
    """air_jit.hip LazyAcc, `++pending[D] == 4`: in-place chains of 1, 3, 4, 5, 8, 9 and 200 terms, `ADDE D,D,T` and `ADDE D,T,D`; and
    find_dot_fusions / LazyAcc::before: two accumulators pending together, D read by a MULE after 5 terms and continued, a term whose
    A or v is another chain's pending accumulator, and the shapes that must not be fused (T aliasing D or A, wholly or in part; T read
    again later; v a word of D or T; A = D) — equal to the reference, which the unfused interpreter equals on the same programs.  One
    program, one compilation."""
    prog = sat_case("chains+guards")[0]
    kern = be.compile_air(prog, SP.N_COLS)
    _run_eval(be, lambda prog, ptrs, pw, den, acc: kern.eval(ptrs, pw, den, LOG_SIZE, LOG_EVAL, acc), sat_case, "chains+guards")
    kern.close()


def test_jit_constraint_runs_on_saturated_operands(be, oracle, sat_case):
    """air_jit.hip, the emitted constraint sum's `++pending == 4`: 9 consecutive CONSTRAINT_B; CONSTRAINT_B / CONSTRAINT_E alternating for 9"""
    prog = sat_case("runs")[0]
    kern = be.compile_air(prog, SP.N_COLS)
    _run_eval(be, lambda prog, ptrs, pw, den, acc: kern.eval(ptrs, pw, den, LOG_SIZE, LOG_EVAL, acc), sat_case, "runs")
    kern.close()


def test_jit_program_cut_into_several_kernels(nz, oracle, sat_case, monkeypatch):
    """Guards + runs under "air.segment" = 200: at least 3 kernels, the materialise-and-restart chain's two roots in different kernels
    (the later one sums the whole chain again: asserted on the text) and the run of 9 CONSTRAINT_B cut in two — every kernel folds on its own count."""
    prog = sat_case("guards+runs")[0]
    monkeypatch.setenv("NX_AIR_SEGMENT", "200")         # the text generator without a context reads the process default
    src = nz.air_source(prog, SP.N_COLS)
    kernels = src.split('extern "C"')[1:]
    assert len(kernels) >= 3
    assert sum(1 for k in kernels if "acc_mad(s0," in k) >= 2 and max(k.count("acc_mad(s0,") for k in kernels) < 9
    assert sum(1 for k in kernels if f"acc_mad(z{prog.marks['D3']}_0," in k) >= 2      # the restarted chain is summed in two kernels
    b = nz.HipBackend(0)
    try:
        b.set_option("air.segment", 200)
        kern = b.compile_air(prog, SP.N_COLS)
        _run_eval(b, lambda prog, ptrs, pw, den, acc: kern.eval(ptrs, pw, den, LOG_SIZE, LOG_EVAL, acc), sat_case, "guards+runs")
        _run_eval(b, lambda prog, ptrs, pw, den, acc: b.eval_constraint_program(prog, ptrs, pw, den, LOG_SIZE, LOG_EVAL, acc), sat_case, "guards+runs")
        kern.close()
    finally:
        b.close()


def test_air_check_on_saturated_programs(be):
    """nx_air_check: the same straight-line bodies (fused chains included) with a vote per constraint, on chains + guards + runs in one
    program.  The roots are built so that they are non-zero on every row; count, first row and value must be the numpy interpreter's.
    The reported value is recomputed on the host, so a wrong device sum would not show in it: every chain root D is therefore followed
    by the root D - K with K the chain's true value, which the device must find zero on every row (it is absent from the report)."""
    from test_trace_check_cpu import interp_check
    prog = SP.all_program(pinned=True, runs=True).program(SP.pinned_chain_econsts())
    n_pinned = 2 * len(SP.CHAIN_TERMS)
    nonzero = [j for j in range(prog.n_constraints) if not (j < 2 * n_pinned and j % 2)]
    cols = np.full((SP.N_COLS, 1 << LOG_SIZE), P - 1, np.uint32)
    want = interp_check(prog, list(cols), LOG_SIZE)
    assert sorted(want) == nonzero and all(w[0] == 1 << LOG_SIZE and w[1] == 0 for w in want.values())
    d = be.columns_from_host(cols)
    rep = be.air_check(prog, _ptrs(d), LOG_SIZE, max_failures=prog.n_constraints)
    assert not rep.ok and rep.n_failed == len(nonzero)
    got = {f.constraint: (f.n_rows, f.first_row, f.value) for f in rep.failures}
    assert got == want
    assert all(v < P for f in rep.failures for v in f.value)


def test_logup_program_on_saturated_chains(be, oracle):
    """nx_logup_program: every chain is the denominator of a FRAC / FRACB (what machine.hip's emit_den writes): the fraction that reads
    the lazy accumulator materialises it; q_norm / q_frac_add / q_inv_from of the logup prelude on what comes out"""
    prog = SP.all_program("frac").program(SP.sat_econsts())
    cols, _ = SP.sat_inputs(prog, 1 << LOG_SIZE)
    want = oracle.logup_program(prog, list(cols), LOG_SIZE, prog.n_logup_cols)
    d = be.columns_from_host(cols)
    got = be.logup_program(prog, _ptrs(d), LOG_SIZE)
    assert len(got) == len(want) == prog.n_logup_cols
    for j, (g, w) in enumerate(zip(got, want)):
        g = g.to_cpu()
        assert _canonical(g) and np.array_equal(g, np.stack(w)), j


# ================================================================ 2. enumerated QM31 products and inverses ===================
def test_enumerated_products_in_interpreter_and_jit(be, oracle):
    """x * y over all 4^8 combinations of {0, 1, p-1, p-2} in the 8 coordinates, times a saturated alpha power: field.cuh's q_mul in the
    interpreter, the prelude's copy in the JIT"""
    prog = SP.mul_program()
    cols = SP.edge_enum(8)
    log_eval, log_size = 16, 15
    pw = np.full((1, 4), P - 1, np.uint32)
    den = np.full(2, P - 1, np.uint32)
    start = np.full((4, 1 << log_eval), P - 1, np.uint32)
    want = SP.accumulate(SP.interp(prog, cols)[0], pw, den, log_size, start)
    assert np.array_equal(want, np.stack(oracle.eval_constraint_program(prog, list(cols), pw, den, log_size, log_eval, acc4=list(start))))
    d = be.columns_from_host(cols)
    acc_i, acc_j = be.columns_from_host(start), be.columns_from_host(start)
    be.eval_constraint_program(prog, _ptrs(d), pw, den, log_size, log_eval, acc_i)
    kern = be.compile_air(prog, 8)
    kern.eval(_ptrs(d), pw, den, log_size, log_eval, acc_j)
    kern.close()
    for got in (acc_i.to_cpu(), acc_j.to_cpu()):
        assert _canonical(got) and np.array_equal(got, want)


def test_enumerated_fractions_in_a_logup_program(be, oracle):
    """FRAC and FRACB with the denominator over all 4^4 combinations — the zero element among them — and numerators from the same set"""
    prog, cols = SP.frac_program(), SP.frac_columns()
    assert not cols[:4, 0].any()
    want = oracle.logup_program(prog, list(cols), 16, 2)
    d = be.columns_from_host(cols)
    got = [g.to_cpu() for g in be.logup_program(prog, _ptrs(d), 16)]
    for g, w in zip(got, want):
        assert _canonical(g) and np.array_equal(g, np.stack(w))
    zero = ~cols[:4].any(axis=0)
    assert zero.sum() == 256 and not got[0][:, zero].any() and not got[1][:, zero].any()     # 0 / 0 and num / 0 contribute 0


def test_built_in_kernels_on_enumerated_operands(be, oracle):
    """logup_finalize_col with one and with two fractions, batch_inverse_qm31 and secure_accumulate over the enumerations"""
    L = oracle.lib()
    cols = SP.edge_enum(8)
    n = cols.shape[1]
    r = np.arange(n)
    mult = np.stack([SP.EDGE[(r ^ (r >> 5)) & 3], SP.EDGE[((r >> 2) + (r >> 9)) & 3]]).astype(np.uint32)
    d_a, d_b = be.columns_from_host(cols[:4]), be.columns_from_host(cols[4:])
    d_m0, d_m1 = be.columns_from_host(mult[0]), be.columns_from_host(mult[1])
    prev = np.full((4, n), P - 1, np.uint32)
    d_prev = be.columns_from_host(prev)
    sa, sb = (P - 1, P - 2, 1, P - 1), (P - 2, 0, P - 1, 1)
    one = be.logup_finalize_col(d_a, scale_a=sa, mult_a=d_m0, prev=d_prev).to_cpu()
    assert _canonical(one) and np.array_equal(one, np.stack(oracle.logup_finalize_col(list(cols[:4]), scale_a=sa, mult_a=mult[0], prev=list(prev))))
    bare = be.logup_finalize_col(d_b, scale_a=SAT4).to_cpu()
    assert _canonical(bare) and np.array_equal(bare, np.stack(oracle.logup_finalize_col(list(cols[4:]), scale_a=SAT4)))
    two = be.logup_finalize_col(d_a, scale_a=sa, mult_a=d_m0, den_b=d_b, scale_b=sb, mult_b=d_m1, prev=d_prev).to_cpu()
    assert _canonical(two) and np.array_equal(two, np.stack(oracle.logup_finalize_col(list(cols[:4]), scale_a=sa, mult_a=mult[0], den_b=list(cols[4:]), scale_b=sb,
                                                                                      mult_b=mult[1], prev=list(prev))))
    acc = be.secure_accumulate(be.columns_from_host(cols[:4]), d_b).to_cpu()
    ref = [np.ascontiguousarray(c).copy() for c in cols[:4]]
    L.orc_secure_accumulate(O.ptr_array(ref), O.ptr_array([np.ascontiguousarray(c) for c in cols[4:]]), C.c_size_t(n))
    assert _canonical(acc) and np.array_equal(acc, np.stack(ref))
    sec = SP.edge_enum(4)
    sec[0, 0] = 1                                      # its contract: never the zero element
    inv = be.batch_inverse_qm31(be.columns_from_host(sec)).to_cpu()
    ref4 = [np.zeros(sec.shape[1], np.uint32) for _ in range(4)]
    L.orc_batch_inverse_qm31(O.ptr_array([np.ascontiguousarray(c) for c in sec]), O.ptr_array(ref4), C.c_size_t(sec.shape[1]))
    assert _canonical(inv) and np.array_equal(inv, np.stack(ref4))


@pytest.mark.parametrize("alpha", [SAT4, (0, 0, 0, P - 1), (P - 1, 0, 0, 0), (1, P - 2, P - 1, 0), (P - 2, P - 2, P - 2, P - 2)])
def test_fri_folds_on_edge_operands(be, oracle, alpha):
    """fold_line and fold_circle_into_line: alpha * t and d * alpha^2 through q_mul with alpha and the columns from EDGE"""
    L = oracle.lib()
    log = 6
    rng = np.random.default_rng(61)
    src = rng.choice(SP.EDGE, size=(4, 1 << log))
    src[:, :4] = P - 1
    dst0 = rng.choice(SP.EDGE, size=(4, 1 << (log - 1)))
    dst0[:, :2] = P - 1
    alpha = np.array(alpha, np.uint32)
    tw = be.precompute_twiddles(log)
    d_src, d_dst = be.columns_from_host(src), be.columns_from_host(dst0)
    be.fold_circle_into_line(tw, d_dst, d_src, alpha)
    ref = [np.ascontiguousarray(c).copy() for c in dst0]
    L.orc_fold_circle_into_line(O.ptr_array(ref), O.ptr_array([np.ascontiguousarray(c) for c in src]), log, O.ptr(alpha))
    got = d_dst.to_cpu()
    assert _canonical(got) and np.array_equal(got, np.stack(ref))
    out = be.fold_line(tw, d_src, alpha, 0).to_cpu()
    ref2 = [np.zeros(1 << (log - 1), np.uint32) for _ in range(4)]
    L.orc_fold_line_dom(O.ptr_array([np.ascontiguousarray(c) for c in src]), log, 0, O.ptr(alpha), O.ptr_array(ref2))
    assert _canonical(out) and np.array_equal(out, np.stack(ref2))


# ================================================================ 3. built-in logup sums ======================================
WIDTHS = (1, 3, 4, 5, 8, 9, 31, 32, 33, 200)
Z_EDGE = (P - 2, 1, 0, P - 1)
# fraction counts 1, 7, 8, 9 and 17 around LOGUP_GROUP = 8; group widths 31, 32 (staged in LDS) and 33, 200 (read where used) around LOGUP_TMAX = 32
FRACTION_SETS = {"1x31": [31], "1x32": [32], "1x33": [33], "1x200": [200], "7": [1, 3, 4, 5, 8, 9, 1], "8": [1, 3, 4, 5, 8, 9, 1, 1],
                 "9": [1, 3, 4, 5, 8, 9, 1, 1, 33], "17": [1, 3, 4, 5, 8, 9, 1, 1, 4, 4, 4, 4, 5, 4, 4, 4, 200]}


@pytest.fixture(scope="module")
def sat_tuples(be):
    log = 6
    host = np.full((200, 1 << log), P - 1, np.uint32)
    ap = np.full((200, 4), P - 1, np.uint32)
    dens = {w: [np.asarray(c) for c in O.logup_combine(list(host[:w]), ap[:w], Z_EDGE)] for w in WIDTHS}
    return log, host, ap, dens


@pytest.mark.parametrize("width", WIDTHS)
def test_logup_combine_and_col_on_saturated_tuples(be, oracle, sat_tuples, width):
    """logup_combine_kernel and tuple_den (logup_col_kernel): `(k & 3) == 3` over SAT tuple columns and SAT alpha powers"""
    log, host, ap, dens = sat_tuples
    d = be.columns_from_host(host[:width])
    got = be.logup_combine(d, ap[:width], Z_EDGE).to_cpu()
    assert _canonical(got) and np.array_equal(got, np.stack(dens[width]))
    mult = np.full(1 << log, P - 1, np.uint32)
    col = be.logup_col(dict(tuple=d, alphas=ap[:width], z=Z_EDGE, scale=SAT4, mult=be.columns_from_host(mult))).to_cpu()
    assert _canonical(col) and np.array_equal(col, np.stack(oracle.logup_finalize_col(dens[width], scale_a=SAT4, mult_a=mult)))
    w2 = WIDTHS[(WIDTHS.index(width) + 3) % len(WIDTHS)]
    two = be.logup_col(dict(tuple=d, alphas=ap[:width], z=Z_EDGE), dict(tuple=be.columns_from_host(host[:w2]), alphas=ap[:w2], z=Z_EDGE, scale=(P - 1, 0, 0, 0))).to_cpu()
    assert _canonical(two) and np.array_equal(two, np.stack(oracle.logup_finalize_col(dens[width], den_b=dens[w2], scale_b=(P - 1, 0, 0, 0))))


@pytest.mark.parametrize("name", list(FRACTION_SETS))
def test_logup_cols_on_saturated_tuples(be, oracle, sat_tuples, name):
    """logup_cols_kernel (nx_logup_cols and nx_logup_cols_batched): the tuple sums of whole groups, staged and direct"""
    log, host, ap, dens = sat_tuples
    widths = FRACTION_SETS[name]
    mult = np.full(1 << log, P - 1, np.uint32)
    d_mult = be.columns_from_host(mult)
    scales = [SAT4 if f % 3 == 0 else (P - 1, 0, 0, 0) if f % 3 == 1 else (1, 0, 0, 0) for f in range(len(widths))]
    fracs = [dict(tuple=be.columns_from_host(host[:w]), alphas=ap[:w], z=Z_EDGE, scale=s, **({"mult": d_mult} if f % 2 else {})) for f, (w, s) in enumerate(zip(widths, scales))]
    want, prev = [], None
    for f, w in enumerate(widths):
        prev = oracle.logup_finalize_col(dens[w], scale_a=scales[f], mult_a=mult if f % 2 else None, prev=prev)
        want.append(np.stack(prev))
    got = be.logup_cols(fracs)
    for f in range(len(widths)):
        g = got[f].to_cpu()
        assert _canonical(g) and np.array_equal(g, want[f]), f
    for j, g in enumerate(be.logup_cols_batched(fracs)):
        assert np.array_equal(g.to_cpu(), want[min(2 * j + 1, len(widths) - 1)]), j


# ================================================================ 4. PCS sums: one factor is derived ===========================
def _points(oracle, seed, n):
    L = oracle.lib()
    ch = C.c_void_p(L.orc_channel_new())
    L.orc_channel_mix_u64(ch, seed)
    pts = []
    for _ in range(n):
        p = np.zeros(8, np.uint32)
        L.orc_get_random_point(ch, O.ptr(p))
        pts.append(p)
    a = np.zeros(4, np.uint32)
    L.orc_channel_draw_secure_felt(ch, O.ptr(a))
    L.orc_channel_free(ch)
    return pts, a


def _oracle_quotients(oracle, cols, alpha, batches):
    log = int(np.log2(cols.shape[1]))
    outs = [np.zeros(1 << log, np.uint32) for _ in range(4)]
    pts = np.concatenate([b[0] for b in batches]).astype(np.uint32)
    counts = np.array([len(b[1]) for b in batches], np.int32)
    cidx = np.array([c for b in batches for c, _ in b[1]], np.int32)
    vals = np.concatenate([v for b in batches for _, v in b[1]]).astype(np.uint32)
    oracle.lib().orc_accumulate_quotients(log, O.ptr_array([np.ascontiguousarray(c) for c in cols]), cols.shape[0], O.ptr(np.asarray(alpha, np.uint32)), len(batches), O.ptr(pts),
                                          O.ptr(counts), O.ptr(cidx), O.ptr(vals), 4, O.ptr_array(outs))
    return np.stack(outs)


@pytest.mark.parametrize("sat_alpha", [False, True])
def test_accumulate_quotients_on_saturated_columns(be, oracle, sat_alpha):
    """quotient_kernel: 430 SAT columns in one batch (86 windows of 5 x 4 coordinates per call, c_k = alpha^k * Im-part factors derived
    by the library) and a second batch of 1, 2, 3 and 5 entries (the tail loop on top of a folded sum); a fresh point per call: 4 calls
    x 344 window-coordinates per alpha family"""
    log, n_cols = 6, 430
    cols = np.full((n_cols, 1 << log), P - 1, np.uint32)
    d = be.columns_from_host(cols)
    rng = np.random.default_rng(430)
    for tail in (1, 2, 3, 5):
        (p1, p2), alpha = _points(oracle, 1000 + tail + 10 * sat_alpha, 2)
        alpha = np.array(SAT4, np.uint32) if sat_alpha else alpha
        batches = [(p1, [(c, rng.integers(0, P, 4, dtype=np.uint32)) for c in range(n_cols)]), (p2, [(c, rng.integers(0, P, 4, dtype=np.uint32)) for c in range(tail)])]
        got = be.accumulate_quotients(d, alpha, batches).to_cpu()
        assert _canonical(got) and np.array_equal(got, _oracle_quotients(oracle, cols, alpha, batches)), tail


@pytest.mark.parametrize("log,n_points", [(17, 18), (11, 4), (12, 4)])
def test_eval_at_points_on_saturated_coefficients(be, oracle, log, n_points):
    """eval_at_point_kernel: SAT coefficients; T_hi comes from the point.  log 17: n_hi = 128 rows of T_hi in one block, 18 points
    (25 windows of 5 x 4 coordinates x 18 = 1800); log 11 and 12: n_hi = 2 (the tail loop alone) and 4 (one 4-step pass)."""
    coeffs = np.full((1, 1 << log), P - 1, np.uint32)
    d = be.columns_from_host(coeffs)
    pts, _ = _points(oracle, 1700 + log, n_points)
    got = be.eval_at_points(d, [0] * n_points, pts)
    assert _canonical(got)
    for i, pt in enumerate(pts):
        assert np.array_equal(got[i], oracle.eval_at_point(coeffs[0], pt)), (log, i)


PAIR_LOGS, PAIRS = (6, 7, 8), 176


@pytest.fixture(scope="module")
def pair_statement(be):
    """Three components of 2^6, 2^7 and 2^8 rows with 176 column pairs each: every column is the oracle's evaluation of the polynomial
    whose coefficients are all p-1, the constraints are a - b = 0 per pair (any values satisfy them).  Returns the trees, the
    components, the oracle session's roots and proof, and the compiled constraint kernel (one for the three components)."""
    import nexus_zkvm_amd.air_program as ap
    trees = [[np.zeros(1 << log, np.uint32) for log in PAIR_LOGS], []]      # tree 0: a (dummy) preprocessed column per component
    comps = []
    pb = ap.ProgramBuilder()
    for k in range(PAIRS):
        (a,), (b,) = pb.next_trace_mask(2 * k), pb.next_trace_mask(2 * k + 1)
        pb.add_constraint(a - b)
    prog = pb.build()
    for i, log in enumerate(PAIR_LOGS):
        col = O.Twiddles(log).evaluate(np.full(1 << log, P - 1, np.uint32), log)
        cols = [(1, 2 * PAIRS * i + k) for k in range(2 * PAIRS)] + [(0, i)]       # the dummy column is claimed, and read by no constraint
        comps.append(ap.Component(log, prog, cols, [[0]] * (2 * PAIRS + 1)))
        trees[1] += [col] * (2 * PAIRS)
    ocfg = O.default_cfg(pow_bits=2)
    so = O.ProverSession(ocfg, max(PAIR_LOGS))
    so.mix_u64(7)
    oroots = [so.commit(t) for t in trees]
    ref = so.prove(comps)
    kern = be.compile_air(prog, 2 * PAIRS + 1)
    yield trees, comps, ocfg, oroots, ref, [kern] * 3
    kern.close()


@pytest.mark.parametrize("coeffs_path", [1, 0])
def test_session_quotients_of_saturated_polynomials(be, nz, pair_statement, coeffs_path):
    """quotient_combine_kernel ("quotients.coeffs" = 1; = 0: the row-wise quotient_kernel on the same statement), reached through a
    prover session.  The coefficient columns are SAT, c_k is derived from alpha and the OODS point; per size group 352 columns go over
    16 slices: 4 windows of 5 per slice and coordinate, 768 window-coordinates in all.  The proof must be the oracle session's, byte for
    byte, for both option values."""
    trees, comps, ocfg, oroots, ref, kernels = pair_statement
    cfg = nz.default_config(pow_bits=int(ocfg[0]), log_blowup=int(ocfg[1]), n_queries=int(ocfg[2]), log_last_layer_degree_bound=int(ocfg[3]), hash_mode=int(ocfg[4]),
                            fri_alpha_mode=int(ocfg[5]), log_constraint_degree=int(ocfg[6]))
    assert be.get_option("quotients.coeffs") == 1
    be.set_option("quotients.coeffs", coeffs_path)
    try:
        sh = be.prover_session(cfg, max(PAIR_LOGS))
        sh.mix_u64(7)
        hroots = [sh.commit(t) for t in trees]
        assert all(np.array_equal(x, y) for x, y in zip(oroots, hroots))
        words = sh.prove(comps, kernels=kernels)
        assert np.array_equal(words, ref)
        sh.close()
    finally:
        be.set_option("quotients.coeffs", 1)


# ================================================================ 5. zero denominators ========================================
def _zero_den_fractions(log):
    """17 fractions over width-1 tuples with alpha^0 = 1 and z = 5: den = t - 5.  t = 5, so den = 0: fractions 0, 3 and 7 of the first
    group on every third row; all 8 of the second group on rows = 1 mod 4; fraction 16 on every row."""
    n = 1 << log
    rng = np.random.default_rng(5)
    rows = np.arange(n)
    tup = rng.integers(6, P, (17, n), dtype=np.uint32)
    for f in (0, 3, 7):
        tup[f, rows % 3 == 0] = 5
    tup[8:16, rows % 4 == 1] = 5
    tup[16, :] = 5
    mult = rng.choice(SP.EDGE[1:], size=(17, n)).astype(np.uint32)
    return tup, mult


def test_zero_denominators_in_logup_cols(be, oracle):
    """logup_cols_kernel: a zero denominator at group positions 0, 3 and 7, in all 8 positions, and on every row — contributes 0 (the
    oracle's qm31_inv(0) is 0) and leaves the other fractions of its group (one m_inv over the group's norms) alone; base-field and
    secure numerators (the two branches that use the inverse norm)"""
    log = 6
    tup, mult = _zero_den_fractions(log)
    one, z = np.array([[1, 0, 0, 0]], np.uint32), (5, 0, 0, 0)
    scales = [(P - 1, 0, 0, 0) if f % 3 == 0 else (5, 6, 7, 8) if f % 3 == 1 else (1, 0, 0, 0) for f in range(17)]
    fracs, want, prev = [], [], None
    for f in range(17):
        fracs.append(dict(tuple=be.columns_from_host(tup[f:f + 1]), alphas=one, z=z, scale=scales[f], mult=be.columns_from_host(mult[f])))
        den = oracle.logup_combine([tup[f]], one, z)
        before = prev
        prev = oracle.logup_finalize_col(den, scale_a=scales[f], mult_a=mult[f], prev=prev)
        want.append(np.stack(prev))
        zero = tup[f] == 5
        assert zero.any() == (f in (0, 3, 7, 16) or 8 <= f < 16)
        if before is not None:                    # the reference itself: a zero denominator adds nothing, any other something
            assert np.array_equal(want[f][:, zero], np.stack(before)[:, zero]) and (want[f][:, ~zero] != np.stack(before)[:, ~zero]).any(axis=0).all()
    got = be.logup_cols(fracs)
    for f in range(17):
        g = got[f].to_cpu()
        assert _canonical(g) and np.array_equal(g, want[f]), f
    for j, g in enumerate(be.logup_cols_batched(fracs)):
        assert np.array_equal(g.to_cpu(), want[min(2 * j + 1, 16)]), j


def test_zero_denominators_in_a_logup_program(be, oracle):
    """the generated fraction kernels (groups of 8 norms under one m_inv): the same 17 fractions declared through the recorder's relation
    API, multiplicities from columns (FRACB)"""
    import nexus_zkvm_amd.air_program as ap
    log = 6
    tup, mult = _zero_den_fractions(log)
    pb = ap.ProgramBuilder()
    rel = pb.relation((5, 0, 0, 0), (3, 1, 4, 1), 1)
    for f in range(17):
        (t,), (m,) = pb.next_trace_mask(f), pb.next_trace_mask(17 + f)
        pb.add_to_relation(rel, m if f % 2 else -m, [t])
    pb.finalize_logup(34, (0, 0, 0, 0))
    prog = pb.build_logup()
    assert prog.n_logup_cols == 17
    cols = [O.u32(c) for c in tup] + [O.u32(c) for c in mult]
    want = oracle.logup_program(prog, cols + [None] * 68, log, 17)
    d = be.columns_from_host(np.stack(cols))
    got = [g.to_cpu() for g in be.logup_program(prog, _ptrs(d) + [None] * 68, log)]
    for f in range(17):
        assert _canonical(got[f]) and np.array_equal(got[f], np.stack(want[f])), f
    assert np.array_equal(got[16], got[15])        # fraction 16: zero on every row


def test_zero_denominators_in_accumulate_quotients(be, oracle):
    """quot_den_inv4: a sample point with coordinates in the base field makes every denominator (Re p.x - d.x) Im p.y - (Re p.y - d.y)
    Im p.x zero on every row: the four norms of a lane are all zero, the quotient is the oracle's (its inverse of 0 is 0)"""
    from test_air_program_cpu import _pt_from_index
    log, n_cols = 6, 9
    rng = np.random.default_rng(66)
    cols = rng.integers(0, P, (n_cols, 1 << log), dtype=np.uint32)
    x, y = _pt_from_index(123456789)
    base_pt = np.array([x, 0, 0, 0, y, 0, 0, 0], np.uint32)
    (p2,), alpha = _points(oracle, 66, 1)
    entries = lambda k: [(c, rng.integers(0, P, 4, dtype=np.uint32)) for c in range(k)]
    d = be.columns_from_host(cols)
    for batches in ([(base_pt, entries(n_cols))], [(p2, entries(5)), (base_pt, entries(n_cols))], [(base_pt, entries(3)), (p2, entries(n_cols))]):
        got = be.accumulate_quotients(d, alpha, batches).to_cpu()
        assert _canonical(got) and np.array_equal(got, _oracle_quotients(oracle, cols, alpha, batches))
    only = be.accumulate_quotients(d, alpha, [(base_pt, entries(n_cols))]).to_cpu()
    assert not only.any()
