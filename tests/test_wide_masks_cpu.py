"""Mask offsets beyond the neighbour row (tests/wide_mask_air.py), the part that needs no GPU.

1. The oracle's row rule, pinned independently of its own index function: the value its interpreter loads at row r, offset o, of a
   2^e-point evaluation is the polynomial at (domain point of r) + o trace steps, the point computed here with circle-group arithmetic and
   the value with eval_at_point.  The same for the trace-domain rule of logup_program and of the checker's reference interpreter.
   This is what makes the oracle a fit reference for tests/test_gpu_wide_masks.py, HUGE (both ends of int32) included.
2. Every statement the GPU file proves is proved by the oracle's session and accepted by the oracle's verifier and by the library's host
   verifier; a flipped word, a trace cell changed at natural row 0 or N - 1 (seen only through the wrap) and a component presented with
   one mask entry altered each fail.
3. Offsets that coincide modulo N are sampled twice, with equal values.
4. The generated kernel text on the host (the stand-alone sanitizer program of tests/test_air_text_host_cpu.py) at STD, FAR(8), HUGE and
   under a segment budget where the last kernel is the first to use an offset.
5. The wide variant has exactly three sample points and enough columns per point for the coefficient quotients."""
import re

import numpy as np
import pytest

import oracle_lib as O
import wide_mask_air as W
import test_air_text_host_cpu as TH
from test_air_program_cpu import denominators
from test_trace_check_cpu import interp_check, natural_row_of_pos, to_natural

P = O.P


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    nexus_zkvm_amd.load_library()
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def ap():
    import nexus_zkvm_amd.air_program as ap
    return ap


def hip_cfg(nz, kw):
    return nz.default_config(pow_bits=kw.get("pow_bits", 10), log_blowup=kw.get("log_blowup", 1), log_constraint_degree=kw.get("log_constraint_degree", 1))


# ---- 0. the helpers of wide_mask_air ------------------------------------------------------------------------------------------------
def test_vectorised_qm31_product_is_the_oracles(oracle):
    rng = np.random.default_rng(1)
    x, y = rng.integers(0, P, (4, 300), dtype=np.uint64), rng.integers(0, P, (4, 300), dtype=np.uint64)
    for k, edge in enumerate((0, 1, P - 1, P - 2)):                      # boundary words in the first rows
        x[:, k], y[:, k] = edge, np.roll([0, 1, P - 1, P - 2], k)
    got = np.stack(W.qmul_rows(list(x), list(y)))
    for i in range(300):
        assert np.array_equal(got[:, i], O.qm31_mul(x[:, i], y[:, i])), i


def test_offset_sets_fit_int32_and_the_sizes_they_are_paired_with():
    for logs, name in W.SESSION_CASES + W.SHARDED_CASES + [W.CONTROL_CASE, W.BOUNDS_CASE[:2]]:
        for l in logs:
            base, sec = W.offsets_of(name, l)
            assert len(base) == 4 and len(sec) == 2 and all(-2 ** 31 <= o < 2 ** 31 for o in base + sec)
    assert all(l == 2 for logs, name in W.SESSION_CASES if name == "COINCIDE" for l in logs)
    assert W.FAR(8) == ((-9, 7, 8, 17), (-8, 11))
    assert {l for logs, _ in W.SESSION_CASES for l in logs} == set(W.SIZES)


@pytest.mark.parametrize("hd,want", [(True, [4, 2, 3, 2, 3]), (False, [2, 2])])
def test_constraint_degrees_of_the_window_component(nz, ap, hd, want):
    c = W.window_component(ap, 5, 0, *W.STD, high_degree=hd)
    assert list(nz.air_constraint_degrees(c.program, len(c.cols))) == want
    assert c.masks[W.COL_A] == list(W.STD[0]) and all(c.masks[W.COL_T + k] == list(W.STD[1]) for k in range(4))
    assert all(c.masks[k] == [0] for k in range(W.N_MAIN) if k != W.COL_A and not W.COL_T <= k < W.COL_T + 4)


# ---- 1. the oracle's row rule ---------------------------------------------------------------------------------------------------------
def _xy(fn, *args):
    out = np.zeros(2, np.uint32)
    fn(*args, O.ptr(out))
    return int(out[0]), int(out[1])


def _padd(p, q):
    return ((p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P)


def _step(n, o):
    """o trace steps of a 2^n-row trace as a circle point: the group has order 2^31, the step is 2^(31 - n); Python integers, no overflow"""
    return _xy(O.lib().orc_circle_point, (int(o) << (31 - n)) % (1 << 31))


class _PolyAt:
    def __init__(self, coeffs):
        self.coeffs, self.seen = coeffs, {}

    def __call__(self, pt):
        if pt not in self.seen:
            v = O.eval_at_point(self.coeffs, [pt[0], 0, 0, 0, pt[1], 0, 0, 0])
            assert not v[1:].any()
            self.seen[pt] = int(v[0])
        return self.seen[pt]


ROW_RULE_OFFSETS = sorted(set(W.ALL_OFFSETS) | {o for part in W.WIDE for o in part} | {W.SEGMENT_LATE, 2})


def _loaded_values(ap, E, n, e):
    """{offset: the 2^e values the oracle's interpreter loads}: one constraint per offset, alpha power e_j, read back from the accumulator
    — the program is the single LOAD, the alpha power 1 and the denominators 1, so the accumulator holds the loaded word itself."""
    out = {}
    for o in ROW_RULE_OFFSETS:
        pb = ap.ProgramBuilder()
        (x,) = pb.next_trace_mask(0, (o,))
        pb.add_constraint(x)
        prog = pb.build()
        assert int(np.int32(np.uint32(prog.instrs[0][3]))) == o
        out[o] = O.eval_constraint_program(prog, [E], [1, 0, 0, 0], np.ones(1 << (e - n), np.uint32), n, e)[0]
    return out


@pytest.mark.parametrize("n,d", [(n, d) for n in (2, 3, 5) for d in (1, 2, 3)])
def test_the_oracles_interpreter_loads_the_polynomial_one_trace_step_further(oracle, ap, n, d):
    e = n + d
    rng = np.random.default_rng(100 * n + d)
    coeffs = rng.integers(0, P, 1 << n, dtype=np.uint32)
    E = O.Twiddles(e).evaluate(coeffs, e)
    f = _PolyAt(coeffs)
    L = O.lib()
    pts = [_xy(L.orc_circle_domain_at, e, L.orc_bit_reverse_index(r, e)) for r in range(1 << e)]
    assert [f(p) for p in pts] == [int(v) for v in E]                       # offset 0: the evaluation is the polynomial at the row's point
    assert len(set(int(v) for v in E)) == 1 << e                            # distinct values: a wrong row cannot pass by accident
    for o, seen in _loaded_values(ap, E, n, e).items():
        s = _step(n, o)
        assert [f(_padd(p, s)) for p in pts] == [int(v) for v in seen], (n, e, o)


@pytest.mark.parametrize("n", [2, 3, 5])
def test_the_trace_domain_rule_of_logup_program_and_of_the_checkers_reference(oracle, ap, n):
    """e = n: a step is +1 in natural coset order.  logup_program: one fraction (a@o) / 1, so the logup column's first coordinate is the
    loaded word.  interp_check (tests/test_trace_check_cpu.py): natural row i reads row (i + o) mod N."""
    rng = np.random.default_rng(7 + n)
    coeffs = rng.integers(0, P, 1 << n, dtype=np.uint32)
    E = O.Twiddles(n).evaluate(coeffs, n)
    f = _PolyAt(coeffs)
    L = O.lib()
    pts = [_xy(L.orc_circle_domain_at, n, L.orc_bit_reverse_index(r, n)) for r in range(1 << n)]
    assert [f(p) for p in pts] == [int(v) for v in E]
    nat = to_natural(E)
    nat_pts = [_xy(L.orc_canonic_coset_at, n, i) for i in range(1 << n)]
    assert [f(p) for p in nat_pts] == [int(v) for v in nat]
    assert [nat_pts[i] for i in natural_row_of_pos(n)] == pts
    for o in ROW_RULE_OFFSETS:
        s = _step(n, o)
        pb = ap.ProgramBuilder()
        (x,) = pb.next_trace_mask(0, (o,))
        one = pb.relation((0, 0, 0, 0), (1, 0, 0, 0), 1)
        pb.add_to_relation(one, x, [1])                                     # x / (1 * 1 - 0)
        pb.finalize_logup(1, (0, 0, 0, 0))
        col = O.logup_program(pb.build_logup(), [E] + [None] * 4, n, 1)[0]
        assert not np.stack(col[1:]).any()
        assert [f(_padd(p, s)) for p in pts] == [int(v) for v in col[0]], (n, o)
        # the checker's reference: the constraint x - c holds on every row iff c is the column one step further, in natural order
        want = np.array([f(_padd(p, s)) for p in nat_pts], np.uint64)
        pb = ap.ProgramBuilder()
        (x,) = pb.next_trace_mask(0, (o,))
        (c,) = pb.next_trace_mask(1)
        pb.add_constraint(x - c)
        assert interp_check(pb.build(), [nat, want], n) == {}, (n, o)


# ---- 2. proving and verifying --------------------------------------------------------------------------------------------------------
class _NoSession:
    """Records nothing: for the component list alone."""

    def mix_u64(self, v):
        pass


def oracle_proof(logs, name, kw, hd, bounds=None, pad=0, tamper=None):
    ocfg = O.default_cfg(**kw)
    run, tree_logs = W.drive(logs, name, lcd=kw["log_constraint_degree"], bounds=bounds, high_degree=hd, pad=pad)
    s = O.ProverSession(ocfg, max(logs))
    roots = []
    comps = run(s, lambda cols: roots.append(s.commit(cols)), tamper=tamper)
    return s.prove(comps), comps, roots, tree_logs, run


def both_verifiers(nz, logs, kw, roots, tree_logs, comps, words):
    """(the oracle verifier's answer, the library's host verifier's answer): None = accepted"""
    v = O.VerifierSession(O.default_cfg(**kw))
    h = nz.VerifierSession(hip_cfg(nz, kw))
    for s in (v, h):
        s.mix_u64(len(logs))
        for r, t in zip(roots, tree_logs):
            s.commit(r, t)
    out = v.verify(comps, words), h.verify(comps, words)
    h.close()
    return out


ALL_CASES = ([(logs, name, cfg, None) for logs, name in W.SESSION_CASES for cfg in W.CONFIGS]
             + [W.BOUNDS_CASE[:2] + ("b1-lcd2", W.BOUNDS_CASE[2])] + [(logs, name, "b1-lcd2", None) for logs, name in W.SHARDED_CASES])


def _case_id(c):
    return f"{'.'.join(map(str, c[0]))}-{c[1]}-{c[2]}" + ("-bounds" if c[3] else "")


@pytest.mark.parametrize("case", ALL_CASES, ids=_case_id)
def test_every_statement_of_the_gpu_file_proves_and_verifies_on_the_host(oracle, nz, case):
    logs, name, cfg, bounds = case
    kw, hd = W.CONFIGS[cfg]
    words, comps, roots, tree_logs, run = oracle_proof(logs, name, kw, hd, bounds)
    assert both_verifiers(nz, logs, kw, roots, tree_logs, comps, words) == (None, None)
    bad = words.copy(); bad[len(bad) // 2] ^= 1
    assert all(e is not None for e in both_verifiers(nz, logs, kw, roots, tree_logs, comps, bad))
    other = run(_NoSession(), lambda cols: None, alter_mask=True)
    assert all(e is not None for e in both_verifiers(nz, logs, kw, roots, tree_logs, other, words))


@pytest.mark.parametrize("logs,name", W.SESSION_CASES, ids=[f"{'.'.join(map(str, l))}-{n}" for l, n in W.SESSION_CASES])
def test_a_cell_seen_only_through_the_wrap_makes_the_oracle_refuse(oracle, logs, name):
    kw, hd = W.CONFIGS["b1-lcd1"]
    for comp in {0, len(logs) - 1}:
        for row in (0, (1 << logs[comp]) - 1):
            with pytest.raises(RuntimeError, match="ConstraintsNotSatisfied"):
                oracle_proof(logs, name, kw, hd, tamper=(comp, row))


def test_the_control_statement_refuses_under_every_configuration(oracle):
    logs, name = W.CONTROL_CASE
    for cfg in W.CONFIGS:
        kw, hd = W.CONFIGS[cfg]
        for row in (0, (1 << logs[0]) - 1):
            with pytest.raises(RuntimeError, match="ConstraintsNotSatisfied"):
                oracle_proof(logs, name, kw, hd, tamper=(0, row))


def test_readers_of_a_cell_are_the_rows_the_reference_checker_names(ap):
    """readers_of against interp_check on the control statement: constraint 0 (w - a0 a3 - a1 - 5 a2) fails exactly on {(r - o) mod N}"""
    logs, name = W.CONTROL_CASE
    base, sec = W.offsets_of(name, logs[0])
    n = 1 << logs[0]
    for row in (0, n - 1):
        nat, _ = W.window_trace(logs[0], 3, base, sec)
        nat[W.COL_A][row] = (int(nat[W.COL_A][row]) + 1) % P
        c = W.window_component(ap, logs[0], 0, base, sec)
        rep = interp_check(c.program, [x.astype(np.uint64) for x in nat], logs[0])
        want = W.readers_of(logs[0], base, row)
        assert set(rep) == {0} and rep[0][:2] == (len(want), want[0]) and len(want) == 4


# ---- 3. coinciding offsets -----------------------------------------------------------------------------------------------------------
def sampled_values(words):
    """NXP1 (oracle/pcs.h proof_serialize): per tree, per column, the sampled values in mask order"""
    w = np.asarray(words, np.uint32)
    i = O.proof_header_words()
    nt = int(w[i]); i += 1 + 8 * nt
    out = []
    for _ in range(nt):
        nc = int(w[i]); i += 1
        tree = []
        for _ in range(nc):
            ns = int(w[i]); i += 1
            tree.append([tuple(int(x) for x in w[i + 4 * s:i + 4 * s + 4]) for s in range(ns)])
            i += 4 * ns
        out.append(tree)
    return out


def test_coinciding_offsets_are_sampled_twice_with_equal_values(oracle, nz):
    kw, hd = W.CONFIGS["b1-lcd1"]
    words, comps, *_ = oracle_proof((2,), "COINCIDE", kw, hd)
    sv = sampled_values(words)
    a = sv[1][W.COL_A]
    assert len(a) == 4 and a[0] == a[1] and a[2] == a[3] and a[0] != a[2]              # (-1, 3 | 4, 0) on four rows
    for k in range(4):
        t = sv[1][W.COL_T + k]
        assert len(t) == 2 and t[0] == t[1]                                            # (0, 4)
    assert all(len(sv[1][k]) == 1 for k in (W.COL_W, W.COL_H3, W.COL_H4))
    # the same statement at STD: four distinct points
    words, *_ = oracle_proof((2,), "STD", kw, hd)
    a = sampled_values(words)[1][W.COL_A]
    assert len(a) == 4 and a[0] != a[3] and a[1] == a[3]                               # -2, -1, 1, 3 on four rows: -1 = 3 there too


# ---- 4. the generated kernel text on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_harness():
    """the compiler of tests/test_air_text_host_cpu.py's harness, resolved once (skips, visibly, only where there is no ROCm compiler)"""
    TH.CLANGXX = TH._clangxx()
    return TH


def _text_case(tmp_path, th, nz, name, prog, n_cols, shapes, seed):
    """The text of `prog` against oracle.eval_constraint_program at every (log_size, log_eval) of `shapes`: random columns, alpha powers and
    start accumulator, the real denominators.  One build per shape (the driver reads the shape from the operand file; the text is the same)."""
    src = nz.air_source(prog, n_cols)
    ec = np.asarray(prog.econsts, np.uint32).reshape(-1, 4)
    n_k = 0
    for log_size, log_eval in shapes:
        rng = np.random.default_rng(seed + 10 * log_size + log_eval)
        n = 1 << log_eval
        cols = rng.integers(0, P, (n_cols, n), dtype=np.uint32)
        pw = rng.integers(0, P, (prog.n_constraints, 4), dtype=np.uint32)
        start = rng.integers(0, P, (4, n), dtype=np.uint32)
        den = denominators(log_size, log_eval)
        want = np.stack(O.eval_constraint_program(prog, list(cols), pw, den, log_size, log_eval, acc4=list(start)))
        header = [n, log_size, log_eval, n_cols, len(ec), prog.n_constraints]
        n_k = th._run_text(tmp_path, f"{name}_{log_size}_{log_eval}", src, False, header, [[cols, ec, pw, den, start, want]])
    return src, n_k


TEXT_SHAPES = [(3, 4), (3, 5), (5, 6)]


@pytest.mark.parametrize("name", ["STD", "FAR8", "HUGE"])
def test_window_text_at_wide_offsets_on_the_host(tmp_path, text_harness, nz, ap, oracle, name):
    base, sec = {"STD": W.STD, "FAR8": W.FAR(8), "HUGE": W.HUGE}[name]
    prog = W.window_program(ap, base, sec)
    src, n_k = _text_case(tmp_path, text_harness, nz, "win" + name, prog, W.N_MAIN, TEXT_SHAPES, 50)
    assert n_k == 1
    declared, used = preamble_and_body_offsets(src.split('extern "C"')[1])
    assert declared == used and len(declared) == len(set(base + sec) | {0})


def preamble_and_body_offsets(kernel):
    """(offset names the kernel's preamble declares, offset names its body uses)"""
    declared = re.findall(r"const u32 (row_\w+) = row_offset\(r, log_size, e, -?\d+\);", kernel)
    assert len(declared) == len(set(declared))
    body = re.sub(r"const u32 row_\w+ = row_offset\([^\n]*\n", "", kernel)
    return set(declared), set(re.findall(r"\brow_[mp]\w+\b", body))


def test_segmented_text_declares_per_kernel_the_offsets_it_uses(tmp_path, text_harness, nz, ap, oracle, monkeypatch):
    """"air.segment" = 200: at least three kernels; offset +3 is first used by the last one."""
    prog = W.segmented_program(ap)
    monkeypatch.setenv("NX_AIR_SEGMENT", str(W.SEGMENT_BUDGET))
    src, n_k = _text_case(tmp_path, text_harness, nz, "winseg", prog, W.N_MAIN, TEXT_SHAPES, 60)
    assert n_k >= 3
    kernels = src.split('extern "C"')[1:]
    per_kernel = [preamble_and_body_offsets(k) for k in kernels]
    for declared, used in per_kernel:
        assert declared == used
    late = f"row_p{W.SEGMENT_LATE}"
    assert [late in d for d, _ in per_kernel] == [False] * (len(kernels) - 1) + [True]
    assert any(len(d) > 1 for d, _ in per_kernel[:-1]) and any(d == {"row_p0"} for d, _ in per_kernel)   # kernels with other offsets, and with the current row alone


# ---- 5. the wide variant ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", W.WIDE_LOGS)
def test_wide_variant_has_three_points_and_enough_columns_for_the_coefficient_path(oracle, nz, log):
    kw, hd = W.CONFIGS["b1-lcd1"]
    run, tree_logs = W.wide_variant(log)
    s = O.ProverSession(O.default_cfg(**kw), log)
    roots = []
    comps = run(s, lambda cols: roots.append(s.commit(cols)))
    points, columns = W.sample_points_of(comps, log)
    n = 1 << log
    assert points == sorted({0, (-2) % n, 3}) and len(points) == 3
    assert columns == sum(len(t) for t in tree_logs) == 1 + W.N_MAIN + W.PAD
    assert columns >= W.COEFFS_COLUMNS_PER_POINT * len(points)
    assert log + kw["log_blowup"] >= kw["log_blowup"] + 2                                # the other condition of csrc/prover.hip's via_coeffs
    words = s.prove(comps)
    assert both_verifiers(nz, (log,), kw, roots, tree_logs, comps, words) == (None, None)
