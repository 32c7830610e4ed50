"""The reference side of the size lattice (tests/size_lattice.py), without a GPU: the lists are what they claim, the CPU oracle proves
every listed statement and its own verifier accepts the proof, and the refusal line — a statement proves iff its smallest component has
log_size >= log_last_layer_degree_bound + 2, else "fri: columns not consumed" — holds on the whole grid.  tests/test_gpu_size_lattice.py
then compares the device with these proofs word for word."""
import itertools
import os

import numpy as np
import pytest

import machine_ref as M
import oracle_lib as O
import size_lattice as S

P = O.P
THREADS = max(4, min(16, os.cpu_count() or 4))
SEED, AD = 31, b"sl"


def test_the_lattice_lists_are_what_they_claim():
    assert S.LADDER == list(range(2, 18))
    # every A in 2 .. 17 occurs as the largest size: alone on the ladder, and from 3 up as the larger size of a pair
    assert {max(logs) for logs in [(L,) for L in S.LADDER]} == set(range(2, 18))
    assert {A for A, _ in S.PAIRS} == set(range(3, 18))
    # every pair up to 15, nothing twice, the larger size first
    assert {(A, B) for A in range(3, 16) for B in range(2, A)} <= set(S.PAIRS)
    assert len(set(S.PAIRS)) == len(S.PAIRS) == 91 + 10 + 10
    assert all(2 <= B < A <= 17 for A, B in S.PAIRS)
    for A in (16, 17):
        assert {2, 5, 6, 7, 10, 11, 12, 13, A - 2, A - 1} <= set(S.pairs_of(A))
    # the groups the GPU file runs are the pairs, each once
    assert sorted((A, B) for A, Bs in S.PAIR_GROUPS for B in Bs) == sorted(S.PAIRS)
    # triples: strictly decreasing, (A, A - 1, A - 2) and (A, 7, 2) for A in {9, 13, 15}, nothing twice
    assert len(set(S.TRIPLES)) == len(S.TRIPLES) and all(a > b > c >= 2 for a, b, c in S.TRIPLES)
    assert {(A, 7, 2) for A in (9, 13, 15)} <= set(S.TRIPLES)
    assert sum(1 for a, b, c in S.TRIPLES if (b, c) == (a - 1, a - 2)) >= 3
    # variants: exactly the (variant, L) on 2 .. 12 the rule lets through, the three last-layer bounds among them
    assert S.VARIANT_LADDER == list(range(2, 13))
    assert {S.VARIANTS[v].get("log_last", 0) for v in S.VARIANTS} == {0, 1, 2, 3}
    want = [(v, L) for v in S.VARIANTS for L in range(2, 13) if L >= S.VARIANTS[v].get("log_last", 0) + 2]
    assert S.VARIANT_CASES == want and len(want) == 10 + 9 + 8 + 11 + 11
    # the commit lattice of A: A alone, every pair of A, the triples led by A; 17 big columns, 1 / 17 small ones by the parity of B
    for A in range(2, 18):
        shapes = S.commit_shapes(A)
        assert shapes[0] == [(A, 17)] and len(shapes) == 1 + len(S.pairs_of(A)) + sum(1 for t in S.TRIPLES if t[0] == A)
        assert all(n == (17 if log & 1 or log == A else 1) for sh in shapes for log, n in sh)
    assert S.SESSION_LOGS == [(L,) for L in range(2, 10)] + [(L, L - 1) for L in range(3, 10)]
    # refusals: the 10 (L, log_last) of the grid below the line, L = 1 included
    assert sorted(S.REFUSED) == sorted((L, ll) for L in range(1, 9) for ll in range(4) if L < ll + 2) and len(S.REFUSED) == 10
    assert (1, 0) in S.REFUSED


def oracle_claimed_sums(comps, cfg, words, seed, ad):
    """`Proof.claimed_sum` of the oracle's proof, recomputed as the reference ships it: the lookup elements drawn from the transcript
    prefix replayed over the proof's own roots, the interaction trace generated from the statement's columns."""
    h = O.proof_header_words()
    roots = [words[h + 1 + 8 * t:h + 9 + 8 * t] for t in range(2)]
    v = O.VerifierSession(cfg)
    for byte in ad:
        v.mix_u64(byte)
    for c in comps:
        v.mix_u64(c[0])
    v.commit(roots[0], [c[0] for c in comps for _ in range(c[1])])
    v.commit(roots[1], [c[0] for c in comps for _ in range(c[2])])
    z, alpha = v.draw_felts(2)
    main, pre = O.synth_tree_columns(comps, 1, seed, threads=THREADS), O.synth_tree_columns(comps, 0, seed, threads=THREADS)
    claimed, off, poff = [], 0, 0
    for c in comps:
        claimed.append(M.interaction_trace(c, main[off:off + c[2]], z, alpha, pre[poff:poff + c[1]])[1])
        off += c[2]; poff += c[1]
    return np.array(claimed, np.uint32)


def prove_and_verify(comps, kw):
    cfg = O.default_cfg(**kw)
    words = M.prove_machine(comps, cfg, seed=SEED, ad=AD, threads=THREADS)
    claimed = oracle_claimed_sums(comps, cfg, words, SEED, AD)
    assert M.verify_machine(comps, cfg, words, claimed, ad=AD) is None, (comps, kw)
    return words, claimed


@pytest.mark.parametrize("config", list(S.LADDER_CONFIGS))
def test_oracle_proves_and_verifies_the_ladder(oracle, config):
    for L in S.LADDER:
        words, claimed = prove_and_verify(S.ladder_statement(L), S.LADDER_CONFIGS[config])
        if L in (2, 3, 9):                 # the verifier is not a rubber stamp at the small end either
            bad = words.copy(); bad[len(bad) // 2] ^= 1
            assert M.verify_machine(S.ladder_statement(L), O.default_cfg(**S.LADDER_CONFIGS[config]), bad, claimed, ad=AD) is not None


@pytest.mark.parametrize("variant", list(S.VARIANTS))
def test_oracle_proves_and_verifies_the_configuration_variants(oracle, variant):
    for v, L in S.VARIANT_CASES:
        if v == variant:
            prove_and_verify(S.ladder_statement(L), S.VARIANTS[v])


def test_oracle_proves_and_verifies_the_synthetic_ladder(oracle):
    cfg = O.default_cfg(**S.SYNTH_CONFIG)
    for L in S.LADDER:
        words = O.prove_synth(S.synth_statement(L), cfg, seed=SEED, ad=AD, threads=THREADS)
        assert O.verify_synth(S.synth_statement(L), cfg, words, ad=AD) is None, L


@pytest.mark.parametrize("A", range(3, 18))
def test_oracle_proves_and_verifies_every_pair(oracle, A):
    for B in S.pairs_of(A):
        prove_and_verify(S.narrow_statement((A, B)), S.NARROW_CONFIG)


def test_oracle_proves_and_verifies_the_triples(oracle):
    for t in S.TRIPLES:
        prove_and_verify(S.narrow_statement(t), S.NARROW_CONFIG)


def test_the_refusal_line_holds_on_the_grid(oracle):
    """log_size >= log_last + 2 and nothing else decides: not the blow-up, not the query count, not the constraint degree.  396 of the
    576 statements prove, 180 are refused with the oracle's message."""
    g = S.GRID
    n_ok = n_refused = 0
    for L, blow, ll, nq, lcd in itertools.product(g["L"], g["log_blowup"], g["log_last"], g["n_queries"], g["log_constraint_degree"]):
        cfg = O.default_cfg(pow_bits=1, log_blowup=blow, n_queries=nq, log_last=ll, log_constraint_degree=lcd)
        comps = S.narrow_statement((L,))
        if S.proves(L, ll):
            assert len(M.prove_machine(comps, cfg, seed=SEED, ad=AD, threads=4)) > 38, (L, blow, ll, nq, lcd)
            n_ok += 1
        else:
            with pytest.raises(RuntimeError, match=S.ORACLE_REFUSAL):
                M.prove_machine(comps, cfg, seed=SEED, ad=AD, threads=4)
            assert (L, ll) in S.REFUSED
            n_refused += 1
    assert (n_ok, n_refused) == (396, 180)


def test_a_statement_is_refused_for_its_smallest_component(oracle):
    """The line is about the SMALLEST component: a large one next to it does not help."""
    cfg = O.default_cfg(pow_bits=1, log_last=2)
    assert len(M.prove_machine(S.narrow_statement((9, 4)), cfg, seed=SEED, ad=AD, threads=4)) > 38
    with pytest.raises(RuntimeError, match=S.ORACLE_REFUSAL):
        M.prove_machine(S.narrow_statement((9, 3)), cfg, seed=SEED, ad=AD, threads=4)
