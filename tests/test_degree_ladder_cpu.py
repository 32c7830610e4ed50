"""The degree ladder (tests/degree_ladder_air.py), the part that needs no GPU.

1. The degree vector of every component kind is the declared one, the mixed component holds every class the planner tells apart, and
   the traces satisfy their constraints under the reference interpreter of tests/test_trace_check_cpu.py.
2. Every statement the GPU file proves is proved by the oracle's session and accepted by the oracle's verifier and by the library's host
   verifier; a flipped word is refused.
3. One changed cell of a result column, for every constraint of the mixed component, makes the oracle refuse.
4. Above the bound (degree 6 at bound 2, degree 4 at bound 1) the oracle refuses: what the GPU file asks of every option setting."""
import numpy as np
import pytest

import degree_ladder_air as D
import oracle_lib as O
from test_trace_check_cpu import interp_check

P = O.P
KINDS = ["d1", "d2", "d3", "d4", "d5", "d6", "low", "mixed"]


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
    return nz.default_config(pow_bits=kw["pow_bits"], log_blowup=kw["log_blowup"], log_constraint_degree=kw["log_constraint_degree"])


# ---- 1. the statement ------------------------------------------------------------------------------------------------------------------
def test_every_form_is_written_at_every_degree_it_reaches():
    by_form = {}
    for name, form, est, true in D.CONSTRAINTS:
        by_form.setdefault(form, []).append((est, true))
    assert by_form["plain"] == [(d, d) for d in range(1, 7)]
    assert by_form["next"] == by_form["prev"] == by_form["top"] == [(d, d) for d in range(1, 6)]
    assert by_form["sel"] == by_form["secb"] == by_form["sece"] == [(d, d) for d in range(2, 6)]          # a flag or T times at least one factor
    assert by_form["over"] == [(5, 4)]
    assert sorted(set(D.degrees_of("mixed"))) == [1, 2, 3, 4, 5] and max(D.degrees_of("low")) == 3
    # form-major order: in the mixed component the classes interleave, no class is one contiguous run
    deg = D.degrees_of("mixed")
    assert all(sum(1 for a, b in zip(deg, deg[1:]) if (a == d) != (b == d)) >= 4 for d in (2, 3, 4, 5))


@pytest.mark.parametrize("kind", KINDS)
def test_degree_vector_is_the_declared_one(nz, ap, kind):
    c = D.ladder_component(ap, kind, 5, 0)
    assert list(nz.air_constraint_degrees(c.program, len(c.cols))) == D.degrees_of(kind)
    assert len(c.cols) == D.n_columns(kind) and c.program.n_constraints == len(D.constraints_of(kind))
    if kind.startswith("d"):
        assert set(D.degrees_of(kind)) == {int(kind[1:])}
    # only the neighbour forms read beyond the current row
    offsets = {o for m in c.masks for o in m}
    assert offsets == ({0, 1, -1} if any(f in ("next", "prev") for _, f, _, _ in D.constraints_of(kind)) else {0})


def test_recorded_ops_cover_the_base_and_both_secure_products(ap):
    import nexus_zkvm_amd.air_program as A
    ops = set(int(op) for op in D.ladder_component(ap, "mixed", 5, 0).program.instrs[:, 0])
    assert {A.MUL, A.MULEB, A.MULE, A.CONSTRAINT_B, A.CONSTRAINT_E} <= ops


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log", [3, 5])
def test_the_trace_satisfies_its_constraints_under_the_reference_interpreter(ap, kind, log):
    nat, _ = D.ladder_trace(kind, log, 11)
    c = D.ladder_component(ap, kind, log, 0)
    assert interp_check(c.program, [x.astype(np.uint64) for x in nat], log) == {}
    assert set(int(v) for v in nat[D.COL_S]) == {0, 1} and set(int(v) for v in nat[D.COL_ONE]) == {1}
    # and a changed result cell is seen by exactly its constraint, on exactly that row
    j = len(D.constraints_of(kind)) - 1
    k, row = D.result_column(kind, j), (1 << log) - 1
    nat[k][row] = (int(nat[k][row]) + 1) % P
    rep = interp_check(c.program, [x.astype(np.uint64) for x in nat], log)
    assert set(rep) == {j} and rep[j][:2] == (1, row)


# ---- 2. proving and verifying ------------------------------------------------------------------------------------------------------------
def oracle_proof(case, tamper=None):
    kw = D.CONFIGS[case[0]]
    run, tree_logs = D.drive(case)
    s = O.ProverSession(O.default_cfg(**kw), max(log for _, log, _ in case[1]))
    roots = []
    comps = run(s, lambda cols: roots.append(s.commit(cols)), tamper=tamper)
    return s.prove(comps), comps, roots, tree_logs


def both_verifiers(nz, case, roots, tree_logs, comps, words):
    """(the oracle verifier's answer, the library's host verifier's answer): None = accepted"""
    kw = D.CONFIGS[case[0]]
    v, h = O.VerifierSession(O.default_cfg(**kw)), nz.VerifierSession(hip_cfg(nz, kw))
    for s in (v, h):
        s.mix_u64(len(case[1]))
        for r, t in zip(roots, tree_logs):
            s.commit(r, t)
    out = v.verify(comps, words), h.verify(comps, words)
    h.close()
    return out


@pytest.mark.parametrize("case", D.PROVABLE_CASES + [D.SWITCH_CASE, D.AFTER_REFUSAL_CASE], ids=D.case_id)
def test_every_case_of_the_gpu_file_proves_and_verifies_on_the_host(oracle, nz, case):
    words, comps, roots, tree_logs = oracle_proof(case)
    assert both_verifiers(nz, case, roots, tree_logs, comps, words) == (None, None)
    bad = words.copy(); bad[len(bad) // 2] ^= 1
    assert all(e is not None for e in both_verifiers(nz, case, roots, tree_logs, comps, bad))


# ---- 3. one changed result cell ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", range(len(D.constraints_of("mixed"))), ids=[c[0] for c in D.constraints_of("mixed")])
def test_one_changed_cell_of_a_result_column_is_refused(oracle, j):
    case = ("b1-lcd2", (("mixed", 4, 0),))
    with pytest.raises(RuntimeError, match="ConstraintsNotSatisfied"):
        oracle_proof(case, tamper=(0, j, (5 * j + 3) % 16))


def test_a_changed_cell_in_the_second_component_of_a_group_is_refused(oracle):
    for comp in (0, 1, 2):
        with pytest.raises(RuntimeError, match="ConstraintsNotSatisfied"):
            oracle_proof(D.GROUP_CASES[1], tamper=(comp, 0, 31))


# ---- 4. above the bound --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.OVER_BOUND_CASES, ids=D.case_id)
def test_a_constraint_above_the_bound_is_refused_by_the_oracle(oracle, case):
    """the quotient has more coefficients than the domain the bound declares has points: the composition the prover commits to is an
    alias, and its value at the out-of-domain point is not the constraints'"""
    with pytest.raises(RuntimeError, match="ConstraintsNotSatisfied"):
        oracle_proof(case)
