"""Mask offsets beyond the neighbour row through every proving path on the device (-m gpu), word for word against the CPU oracle.

The statement is tests/wide_mask_air.py: a base-field column read at four offsets and a secure column read at two, from the sets STD
(-2, -1, 1, 3 | -3, 2), FAR(N) (every offset wraps an N-row trace at least once), COINCIDE (two pairs of mask entries share a point on four
rows) and HUGE (both ends of int32).  tests/test_wide_masks_cpu.py pins the oracle's row rule at every one of these offsets against
plain point arithmetic, and proves and verifies every statement below on the host.

a. the composition kernels directly: nx_eval_constraint_program and nx_air_compile + nx_air_eval (both copies of row_offset) at
   log_size {2, 3, 5, 9} x log_eval - log_size {1, 2, 3}, the "air.segment" = 200 program whose last kernel is the first to use an offset.
b. whole proofs through the session: bytes and channel digest of the oracle's session under half-domain on / off, quarter-domain x
   degree-split, blow-up 2, per-component bounds (compute_composition's shortcuts, GenericAir::mask_points, the by-point quotient batches,
   the host OODS check).
c. three sample points through the coefficient quotients ("quotients.coeffs"), which otherwise only ever ran with two.
d. row-sharded: masked columns are all-gathered whole; 2 and 4 thread-ranks give the single-GPU bytes.
e. nx_logup_program reading relation values and a multiplicity at offsets.
f. the control: a cell that is read only through the wrap makes every strategy refuse, and nx_prover_check names the rows."""
import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import oracle_lib as O
import wide_mask_air as W
from test_air_program_cpu import denominators
from test_gpu_machine import _run_ranks
from test_gpu_options import backend_with

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


def hip_cfg(nz, kw):
    return nz.default_config(pow_bits=kw["pow_bits"], log_blowup=kw["log_blowup"], log_constraint_degree=kw["log_constraint_degree"])


class Contexts:
    """One context per option set, made on first use and kept for the module: a context compiles a recorded program once (the kernel
    cache of csrc/prover.hip is per context), so the statements of one option set share their kernels.  The shared `be` keeps its defaults."""

    def __init__(self, nz):
        self.nz, self.made = nz, {}

    def get(self, options):
        key = tuple(sorted(options.items()))
        if key not in self.made:
            self.made[key] = backend_with(self.nz, options)
        return self.made[key]

    def close(self):
        for b in self.made.values():
            b.close()
        self.made.clear()


@pytest.fixture(scope="module")
def contexts(nz):
    c = Contexts(nz)
    yield c
    c.close()


class OracleProofs:
    """The oracle's side of every statement, computed once: (proof words, channel digest after the proof, roots, tree_logs)."""

    def __init__(self):
        self.refs = {}

    def get(self, logs, name, cfg, bounds=None, pad=0):
        key = (logs, name, cfg, bounds, pad)
        if key not in self.refs:
            kw, hd = W.CONFIGS[cfg]
            run, tree_logs = W.drive(logs, name, lcd=kw["log_constraint_degree"], bounds=bounds, high_degree=hd, pad=pad)
            s = O.ProverSession(O.default_cfg(**kw), max(logs))
            roots = []
            comps = run(s, lambda cols: roots.append(s.commit(cols)))
            words = s.prove(comps)
            words.setflags(write=False)
            self.refs[key] = (words, s.digest(), roots, tree_logs)
        return self.refs[key]


@pytest.fixture(scope="module")
def refs(oracle):
    r = OracleProofs()
    yield r
    r.refs.clear()


def same_words(ref, words, what):
    assert len(ref) == len(words), (what, len(ref), len(words))
    if not np.array_equal(ref, words):
        pytest.fail(f"{what}: first differing proof word {int(np.nonzero(ref != words)[0][0])} of {len(ref)}")


# ---- a. the composition kernels ---------------------------------------------------------------------------------------------------
RANDOM_COLS, RANDOM_OPS = 12, 120


def kernel_programs(ap):
    """name -> (program, column count): three window programs and a random one that uses every opcode, masks from every offset list"""
    progs = {"window-STD": (W.window_program(ap, *W.STD), W.N_MAIN), "window-FAR8": (W.window_program(ap, *W.FAR(8)), W.N_MAIN),
             "window-HUGE": (W.window_program(ap, *W.HUGE), W.N_MAIN)}
    stride = W.ALL_OFFSETS[::3] + W.ALL_OFFSETS[1::3] + W.ALL_OFFSETS[2::3]           # neighbours in the list are far apart in value
    progs["random"] = (W.random_program(ap, np.random.default_rng(77), RANDOM_COLS, RANDOM_OPS, stride), RANDOM_COLS)
    return progs


@pytest.fixture(scope="module")
def compiled(be, ap):
    """every program compiled once (hiprtc); the shapes below share the kernels"""
    progs = kernel_programs(ap)
    kernels = {name: be.compile_air(prog, n_cols) for name, (prog, n_cols) in progs.items()}
    yield progs, kernels
    for k in kernels.values():
        k.close()


@pytest.fixture(scope="module")
def segmented(contexts, ap):
    b = contexts.get({"air.segment": W.SEGMENT_BUDGET})
    prog = W.segmented_program(ap)
    k = b.compile_air(prog, W.N_MAIN)
    yield b, prog, k
    k.close()


def composition_case(b, prog, n_cols, kernel, log, e, seed, interpreter=True):
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, P, (n_cols, 1 << e), dtype=np.uint32)
    pw = rng.integers(0, P, (prog.n_constraints, 4), dtype=np.uint32)
    start = rng.integers(0, P, (4, 1 << e), dtype=np.uint32)                   # the accumulator is added to, not overwritten
    den = denominators(log, e)
    want = np.stack(O.eval_constraint_program(prog, list(cols), pw, den, log, e, acc4=list(start)))
    d_cols = b.columns_from_host(cols)
    ptrs = [d_cols.ptr.value + k * (4 << e) for k in range(n_cols)]
    acc = b.columns_from_host(start)
    kernel.eval(ptrs, pw, den, log, e, acc)
    jit = acc.to_cpu()
    acc.free()
    got = None
    if interpreter:
        acc = b.columns_from_host(start)
        b.eval_constraint_program(prog, ptrs, pw, den, log, e, acc)
        got = acc.to_cpu()
        acc.free()
    d_cols.free()
    return want, jit, got


@pytest.mark.parametrize("log,d", W.KERNEL_SHAPES, ids=[f"log{l}-plus{d}" for l, d in W.KERNEL_SHAPES])
def test_composition_kernels_at_wide_offsets(be, oracle, compiled, segmented, log, d):
    """row_offset of csrc/constraints.hip (the interpreter) and of the JIT prelude in csrc/air_jit.hip against the oracle's int64 rule;
    at log 2 and 3 most offsets wrap, FAR(8) and HUGE wrap at every size."""
    progs, kernels = compiled
    for name, (prog, n_cols) in progs.items():
        want, jit, interp = composition_case(be, prog, n_cols, kernels[name], log, log + d, 1000 + 10 * log + d)
        assert np.array_equal(interp, want), (name, "nx_eval_constraint_program")
        assert np.array_equal(jit, want), (name, "nx_air_eval")
    b, prog, k = segmented
    want, jit, interp = composition_case(b, prog, W.N_MAIN, k, log, log + d, 2000 + 10 * log + d)
    assert np.array_equal(jit, want), "nx_air_eval, segmented"
    assert np.array_equal(interp, want), "nx_eval_constraint_program, the segmented program"


def test_segmented_program_is_several_kernels(nz, ap, monkeypatch):
    monkeypatch.setenv("NX_AIR_SEGMENT", str(W.SEGMENT_BUDGET))
    assert nz.air_source(W.segmented_program(ap), W.N_MAIN).count('extern "C"') >= 3


# ---- b. whole proofs through the session ------------------------------------------------------------------------------------------
# name -> (configuration of wide_mask_air.CONFIGS, context options)
STRATEGIES = {
    "half0": ("b1-lcd1", {"air.half_domain": 0}),
    "half1": ("b1-lcd1", {"air.half_domain": 1}),
    **{f"quarter{q}-split{s}": ("b1-lcd2", {"air.quarter_domain": q, "air.degree_split": s}) for q in (0, 1, 2) for s in (0, 1)},
    "blowup2-split0": ("b2-lcd2", {"air.degree_split": 0}),
    "blowup2-split1": ("b2-lcd2", {"air.degree_split": 1}),
}


def session_matches(b, nz, refs, logs, name, cfg, bounds=None, pad=0, verify=True):
    kw, hd = W.CONFIGS[cfg]
    ref, digest, oroots, tree_logs = refs.get(logs, name, cfg, bounds, pad)
    run, _ = W.drive(logs, name, lcd=kw["log_constraint_degree"], bounds=bounds, high_degree=hd, pad=pad)
    s = b.prover_session(hip_cfg(nz, kw), max(logs))
    try:
        roots = []
        comps = run(s, lambda cols: roots.append(s.commit(cols)))
        assert all(np.array_equal(x, y) for x, y in zip(oroots, roots)), (logs, name, "roots")
        words = s.prove(comps)
        same_words(ref, words, (logs, name, cfg))
        assert np.array_equal(s.digest(), digest), (logs, name, "channel digest")
    finally:
        s.close()
    if verify:
        for bad in (False, True):
            w = words.copy()
            if bad:
                w[len(w) // 2] ^= 1
            v, h = O.VerifierSession(O.default_cfg(**kw)), nz.VerifierSession(hip_cfg(nz, kw))
            for vs in (v, h):
                vs.mix_u64(len(logs))
                for r, t in zip(roots, tree_logs):
                    vs.commit(r, t)
            assert (v.verify(comps, w) is None) == (not bad) and (h.verify(comps, w) is None) == (not bad), (logs, name, "flipped" if bad else "accepted")
            h.close()
    return words


@pytest.mark.parametrize("strategy", list(STRATEGIES))
@pytest.mark.parametrize("logs,name", W.SESSION_CASES, ids=[f"{'.'.join(map(str, l))}-{n}" for l, n in W.SESSION_CASES])
def test_session_proofs_at_wide_offsets_are_the_oracles(contexts, nz, refs, logs, name, strategy):
    """3 and 4 straddle the line from which the half- and quarter-domain shortcuts apply; (2,) is where offsets coincide; in (5, 2),
    (3, 4, 5) and (7, 4) the quotient batches of several sizes each hold 3 to 7 points."""
    cfg, options = STRATEGIES[strategy]
    session_matches(contexts.get(options), nz, refs, logs, name, cfg)


@pytest.mark.parametrize("strategy", ["quarter2-split1", "quarter0-split0"])
def test_session_with_per_component_bounds(contexts, nz, refs, strategy):
    logs, name, bounds = W.BOUNDS_CASE
    cfg, options = STRATEGIES[strategy]
    session_matches(contexts.get(options), nz, refs, logs, name, cfg, bounds=bounds)


# ---- c. three sample points through the coefficient quotients ------------------------------------------------------------------------
@pytest.mark.parametrize("coeffs", [0, 1])
@pytest.mark.parametrize("log", W.WIDE_LOGS)
def test_three_sample_points_through_the_coefficient_quotients(contexts, nz, refs, log, coeffs):
    """accumulate_quotients_coeffs is taken when columns >= 48 x points: 145 columns, points 0, -2, +3 (the CPU file asserts both)"""
    session_matches(contexts.get({"quotients.coeffs": coeffs}), nz, refs, (log,), "WIDE", "b1-lcd1", pad=W.PAD, verify=False)


# ---- d. row-sharded ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,quarter,case", [(2, 2, 0), (4, 2, 0), (2, 0, 0), (4, 0, 0), (2, 2, 1)],
                         ids=["2ranks-quarter2-9", "4ranks-quarter2-9", "2ranks-quarter0-9", "4ranks-quarter0-9", "2ranks-quarter2-7.4"])
def test_row_sharded_proofs_at_wide_offsets(be, nz, refs, world, quarter, case):
    """columns read at a non-zero offset are all-gathered whole (columns_on_eval_domain, the `nm` branch of the sharded quarter domain):
    every rank returns the single-GPU bytes, which are the oracle's"""
    logs, name = W.SHARDED_CASES[case]
    cfg = "b1-lcd2"
    kw, hd = W.CONFIGS[cfg]
    ref = refs.get(logs, name, cfg)[0]
    same_words(ref, session_matches(be, nz, refs, logs, name, cfg, verify=False), "single GPU")
    run, _ = W.drive(logs, name, lcd=kw["log_constraint_degree"], high_degree=hd)

    def fn(b, comm, rank):
        b.set_option("air.quarter_domain", quarter)
        ss = b.prover_session(hip_cfg(nz, kw), max(logs))
        ss.set_comm(comm)
        try:
            return ss.prove(run(ss, ss.commit))
        finally:
            ss.close()
    for r, w in enumerate(_run_ranks(nz, world, fn)):
        same_words(ref, w, (world, quarter, logs, "rank", r))


# ---- e. nx_logup_program at offsets -----------------------------------------------------------------------------------------------------
LOGUP_FILLERS = 10


@pytest.mark.parametrize("log,segment", [(2, None), (3, None), (6, None), (6, 200)])
def test_logup_program_reads_relation_values_at_offsets(contexts, nz, ap, oracle, log, segment, monkeypatch):
    """tuple values at a@-2 and a@+3, a multiplicity expression reading q@-3 (on four rows -2 and +3 wrap onto the window's own rows);
    with "air.segment" = 200 the program is several kernels"""
    import air_examples as AE
    rng = np.random.default_rng(40 + log)
    z, alpha = rng.integers(0, P, 4, dtype=np.uint32), rng.integers(0, P, 4, dtype=np.uint32)
    nat, fin = AE.relation_main_trace(log, 600 + log)
    frac = W.relation_program_at_offsets(ap, z, alpha, (0, 0, 0, 0), LOGUP_FILLERS).build_logup()
    n_in = AE.RELATION_COLS
    want = oracle.logup_program(frac, fin + [None] * (4 * frac.n_logup_cols), log, frac.n_logup_cols)
    if segment:
        monkeypatch.setenv("NX_AIR_SEGMENT", str(segment))
        assert nz.logup_program_source(frac, n_in + 4 * frac.n_logup_cols, frac.n_logup_cols).count("__attribute__((global))") >= 2
        monkeypatch.delenv("NX_AIR_SEGMENT")
    b = contexts.get({"air.segment": segment} if segment else {})
    d = b.columns_from_host(np.stack(fin))
    ptrs = [d.ptr.value + k * (4 << log) for k in range(n_in)] + [None] * (4 * frac.n_logup_cols)
    got = b.logup_program(frac, ptrs, log)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.to_cpu(), np.stack(w)), (log, segment, "logup column", j)
    d.free()


# ---- f. the control: the offsets matter -------------------------------------------------------------------------------------------------
CONTROL_STRATEGIES = ["half1", "half0", "quarter2-split1", "blowup2-split0"]


@pytest.mark.parametrize("strategy", CONTROL_STRATEGIES)
def test_a_cell_read_only_through_the_wrap_is_refused_under_every_strategy(contexts, nz, refs, strategy):
    """One cell of `a` changed at natural row 0 and, in a separate run, at row N - 1: no constraint reads `a` at offset 0, so the cell is
    seen only by rows (r - o) mod N.  A prover that ignored the offsets would not notice.  The context then proves the untouched statement."""
    logs, name = W.CONTROL_CASE
    cfg, options = STRATEGIES[strategy]
    kw, hd = W.CONFIGS[cfg]
    b = contexts.get(options)
    run, _ = W.drive(logs, name, lcd=kw["log_constraint_degree"], high_degree=hd)
    for row in (0, (1 << logs[0]) - 1):
        s = b.prover_session(hip_cfg(nz, kw), logs[0])
        try:
            comps = run(s, s.commit, tamper=(0, row))
            with pytest.raises(nz.NexusHipError, match="ConstraintsNotSatisfied"):
                s.prove(comps)
        finally:
            s.close()
    session_matches(b, nz, refs, logs, name, cfg, verify=False)


@pytest.mark.parametrize("row", [0, 31])
def test_the_checker_names_the_rows_that_read_the_cell(be, nz, row):
    """nx_prover_check on the control statement: constraint 0 (w - a0 a3 - a1 - 5 a2) fails on exactly the four rows {(row - o) mod N},
    nothing else fails (tests/test_wide_masks_cpu.py ties readers_of to the reference interpreter)"""
    logs, name = W.CONTROL_CASE
    kw, hd = W.CONFIGS["b1-lcd1"]
    base, _ = W.offsets_of(name, logs[0])
    readers = W.readers_of(logs[0], base, row)
    run, _ = W.drive(logs, name)
    s = be.prover_session(hip_cfg(nz, kw), logs[0])
    try:
        comps = run(s, s.commit, tamper=(0, row))
        rep = s.check(comps)
        assert [(f.component, f.constraint, f.first_row, f.n_rows) for f in rep.failures] == [(0, 0, readers[0], len(readers))] and rep.n_failed == 1
        assert len(readers) == 4 and row not in readers
    finally:
        s.close()
    s = be.prover_session(hip_cfg(nz, kw), logs[0])
    try:
        assert s.check(run(s, s.commit)).ok
    finally:
        s.close()
