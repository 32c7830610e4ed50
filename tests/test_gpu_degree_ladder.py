"""The composition shortcuts at every constraint degree on the device (-m gpu), word for word against the CPU oracle.

The statement is tests/degree_ladder_air.py: one constraint per degree 1 .. 5 in every form the planner of csrc/prover.hip
(prepare_component_kernels) tells apart — plain products, a selector times a sum, a factor at the next and at the previous row, secure
times base and secure times secure, a top term beside lower ones, and a product whose estimated degree (5) exceeds its true one (4).
tests/test_degree_ladder_cpu.py proves and verifies every statement below on the host; tests/test_exact_algebra_cpu.py states which degree
each shortcut is exact for (half domain: 2, the 2N-point domain: 3, 3N + 1 samples: 4, the 4N-point domain: 5).

a. every case under every combination of "air.quarter_domain" {0, 1, 2} x "air.half_domain" {0, 1} x "air.degree_split" {0, 1}: proof
   words and channel digest are the oracle session's.  Sizes 2^3 (below the line from which the shortcuts apply), 2^4 (at it), 2^5 and
   2^10 (several blocks per kernel), each with only degree 4, only degree 5 and all degrees mixed; blowup 1 / bound 1, blowup 2 / bound 2,
   per-component bounds; two components of one size that share a quarter group, one on the quarter and one on the full domain, alone and
   beside a bound-1 component whose domain has the same size.
b. the mixed component once more without the coefficient quotients and with its kernels cut into segments.
c. row-sharded on two thread-ranks.
d. above the bound — degree 6 at bound 2, degree 4 at bound 1 — no option setting returns a proof, and the context is left usable.

The field is exact: equality is of words, there is no tolerance anywhere."""
import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import degree_ladder_air as D
import oracle_lib as O
from test_gpu_machine import _run_ranks
from test_gpu_options import backend_with

pytestmark = pytest.mark.gpu
NX_ERR_PROTOCOL = -4
OPTION_NAMES = ("air.quarter_domain", "air.half_domain", "air.degree_split")
OPTION_PRODUCT = [(q, h, s) for q in (0, 1, 2) for h in (0, 1) for s in (0, 1)]


def option_id(o):
    return f"quarter{o[0]}-half{o[1]}-split{o[2]}"


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


@pytest.fixture
def with_options(be):
    """sets the three composition options on the shared context for one test; its defaults come back afterwards, also when the test fails"""
    defaults = {name: be.get_option(name) for name in OPTION_NAMES}

    def set_options(values):
        for name, v in zip(OPTION_NAMES, values):
            be.set_option(name, v)
            assert be.get_option(name) == v
    yield set_options
    for name, v in defaults.items():
        be.set_option(name, v)


def hip_cfg(nz, kw):
    return nz.default_config(pow_bits=kw["pow_bits"], log_blowup=kw["log_blowup"], log_constraint_degree=kw["log_constraint_degree"])


def max_log(case):
    return max(log for _, log, _ in case[1])


class OracleProofs:
    """The oracle's side of every case, computed once: (proof words, channel digest after the proof, roots)."""

    def __init__(self):
        self.refs = {}

    def get(self, case):
        if case not in self.refs:
            run, _ = D.drive(case)
            s = O.ProverSession(O.default_cfg(**D.CONFIGS[case[0]]), max_log(case))
            roots = []
            comps = run(s, lambda cols: roots.append(s.commit(cols)))
            words = s.prove(comps)
            words.setflags(write=False)
            self.refs[case] = (words, s.digest(), roots)
        return self.refs[case]


@pytest.fixture(scope="module")
def refs(oracle):
    r = OracleProofs()
    yield r
    r.refs.clear()


def same_words(ref, words, what):
    assert len(ref) == len(words), (what, len(ref), len(words))
    if not np.array_equal(ref, words):
        pytest.fail(f"{what}: first differing proof word {int(np.nonzero(ref != words)[0][0])} of {len(ref)}")


def session_matches(b, nz, refs, case, comm=None):
    """the case proved on context `b` under its current options: roots, proof words and channel digest are the oracle's"""
    ref, digest, oroots = refs.get(case)
    run, _ = D.drive(case)
    s = b.prover_session(hip_cfg(nz, D.CONFIGS[case[0]]), max_log(case))
    try:
        if comm is not None:
            s.set_comm(comm)
        roots = []
        comps = run(s, lambda cols: roots.append(s.commit(cols)))
        assert all(np.array_equal(x, y) for x, y in zip(oroots, roots)), (D.case_id(case), "roots")
        words = s.prove(comps)
        same_words(ref, words, D.case_id(case))
        assert np.array_equal(s.digest(), digest), (D.case_id(case), "channel digest")
    finally:
        s.close()
    return words


# ---- a. every case under every option combination -----------------------------------------------------------------------------------
@pytest.mark.parametrize("options", OPTION_PRODUCT, ids=option_id)
@pytest.mark.parametrize("case", D.SIZE_CASES, ids=D.case_id)
def test_sizes_at_degree_four_five_and_mixed(be, nz, refs, with_options, case, options):
    """2^3: everything is evaluated whole; 2^4: the first size with a half and a quarter; 2^10: more than one block per kernel.  Only
    degree 4 (the quarter's class), only degree 5 (fills the 4N-point space: the component's own domain) and all degrees interleaved, so
    that under the default options the half, low, quarter and full parts are all non-empty at once."""
    with_options(options)
    session_matches(be, nz, refs, case)


@pytest.mark.parametrize("options", OPTION_PRODUCT, ids=option_id)
@pytest.mark.parametrize("case", D.SINGLE_DEGREE_CASES, ids=D.case_id)
def test_single_low_degrees(be, nz, refs, with_options, case, options):
    """only degree 1, only degree 2, only degree 3: one class each, nothing for the quarter to take"""
    with_options(options)
    session_matches(be, nz, refs, case)


@pytest.mark.parametrize("options", OPTION_PRODUCT, ids=option_id)
@pytest.mark.parametrize("case", D.CONFIG_CASES, ids=D.case_id)
def test_other_configurations(be, nz, refs, with_options, case, options):
    """blowup 1 / bound 1 (degrees <= 3 only), blowup 2 / bound 2 (the committed domain is the 4N-point one: no quarter, no half) and
    per-component bounds (2, 1) on sizes (5, 4)"""
    with_options(options)
    session_matches(be, nz, refs, case)


@pytest.mark.parametrize("options", OPTION_PRODUCT, ids=option_id)
@pytest.mark.parametrize("case", D.GROUP_CASES, ids=D.case_id)
def test_a_quarter_part_and_a_full_part_in_one_size_group(be, nz, refs, with_options, case, options):
    """The quarter groups are keyed by size: a degree-4 component (on the quarter) and a degree-5 component (on its own domain) of one
    size, alone and beside a bound-1 component of twice the rows, whose own domain is as large as theirs."""
    with_options(options)
    session_matches(be, nz, refs, case)


# ---- b. other switches -----------------------------------------------------------------------------------------------------------------
def test_mixed_without_the_coefficient_quotients(nz, refs):
    """a context of its own with "quotients.coeffs" = 0 (70 columns at three sample points stay below the width from which the
    coefficient route is taken, so this pins that the switch changes nothing else on the way)"""
    b = backend_with(nz, {"quotients.coeffs": 0})
    try:
        session_matches(b, nz, refs, D.SWITCH_CASE)
    finally:
        b.close()


def test_mixed_with_every_part_cut_into_segments(nz, refs, monkeypatch):
    """"air.segment" = 200: the half, low, quarter and full parts of the mixed component are several kernels each"""
    import nexus_zkvm_amd.air_program as ap
    c = D.ladder_component(ap, "mixed", 5, 0)
    monkeypatch.setenv("NX_AIR_SEGMENT", str(D.SEGMENT_BUDGET))
    assert nz.air_source(c.program, len(c.cols)).count('extern "C"') >= 4
    monkeypatch.delenv("NX_AIR_SEGMENT")
    b = backend_with(nz, {"air.segment": D.SEGMENT_BUDGET})
    try:
        session_matches(b, nz, refs, D.SWITCH_CASE)
    finally:
        b.close()


# ---- c. row-sharded ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quarter", [2, 0])
def test_row_sharded_mixed_degrees(be, nz, refs, quarter):
    """2 thread-ranks: the degree-4 part's columns come from an N-point transform on their owner, the degree-5 part's from the 4N-point
    one; every rank returns the single-GPU words, which are the oracle's"""
    case = D.SHARDED_CASE
    ref = refs.get(case)[0]
    session_matches(be, nz, refs, case)

    def fn(b, comm, rank):
        b.set_option("air.quarter_domain", quarter)
        run, _ = D.drive(case)
        ss = b.prover_session(hip_cfg(nz, D.CONFIGS[case[0]]), max_log(case))
        ss.set_comm(comm)
        try:
            return ss.prove(run(ss, ss.commit))
        finally:
            ss.close()
    for r, w in enumerate(_run_ranks(nz, 2, fn)):
        same_words(ref, w, (quarter, "rank", r))


# ---- d. above the bound ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.OVER_BOUND_CASES, ids=D.case_id)
def test_above_the_bound_no_setting_returns_a_proof(be, nz, refs, with_options, case):
    """A degree-6 constraint at bound 2 and a degree-4 constraint at bound 1: the quotient does not fit the domain the bound declares.
    Whatever the shortcuts assemble, the OODS check refuses it (NX_ERR_PROTOCOL), under every option setting; the context then proves a
    valid case and holds no more device memory than before."""
    session_matches(be, nz, refs, D.AFTER_REFUSAL_CASE)          # the per-context tables this size needs exist before the count is taken
    be.sync()
    live0, _ = be.memory(reset_peak=True)
    run, _ = D.drive(case)
    for options in OPTION_PRODUCT:
        with_options(options)
        s = be.prover_session(hip_cfg(nz, D.CONFIGS[case[0]]), max_log(case))
        try:
            comps = run(s, s.commit)
            with pytest.raises(nz.NexusHipError, match=rf"error {NX_ERR_PROTOCOL}: .*ConstraintsNotSatisfied"):
                s.prove(comps)
        finally:
            s.close()
    with_options(OPTION_PRODUCT[-1])
    session_matches(be, nz, refs, D.AFTER_REFUSAL_CASE)
    be.sync()
    live1, _ = be.memory()
    assert live1 == live0
