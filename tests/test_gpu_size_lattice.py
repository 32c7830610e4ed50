"""Proofs and commits at every size 2^2 .. 2^17, alone and in pairs, on the device (-m gpu), bit-exact against the CPU oracle.

Which kernel runs, and how often, is decided by the log sizes of a statement (tests/size_lattice.py names the thresholds); the other
GPU files sweep the options and the AIR forms at a dozen sizes, this one sweeps the sizes.

1. Commit lattice: for every largest size A — A alone, A with every paired B, the triples led by A — in both hash modes: the roots of
   nx_commit_root (and of nx_lde_commit, A alone) against oracle_lib.lde_commit, every layer of nx_merkle_commit on the extended columns
   against the oracle's tree.  The stage-level part: a proof mismatch below can be localised here.
2. Proof lattice: nx_prove_machine word for word on the ladder (two configurations, the library's verifier accepts and refuses a flipped
   word), on every pair and triple, under the last-layer / blow-up / query-count variants; nx_prove_synth on the ladder.
3. Session ladder: the recorded logup AIR with mask offsets -1 / 0 / +1 down to 4- and 8-row traces.
4. Refusals, mirrored: below log_size = log_last + 2 the library answers NX_ERR_PROTOCOL "... not consumed" where the oracle throws
   "fri: columns not consumed", leaves nothing allocated and proves the next statement.
5. Primitives at sizes the lattice cannot localise, direct calls against the oracle's functions."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import machine_ref as M
import oracle_lib as O
import size_lattice as S

pytestmark = pytest.mark.gpu
P = O.P
THREADS = max(4, min(16, os.cpu_count() or 4))
SEED, AD = 31, b"sl"
MAX_LOG = max(S.LADDER)


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


def _same(ref, words, what=None):
    assert len(ref) == len(words), (what, len(ref), len(words))
    if not np.array_equal(ref, words):
        bad = int(np.nonzero(ref != words)[0][0])
        pytest.fail(f"{what}: first differing proof word {bad} of {len(ref)} (roots are words 6..37)")


def assert_same_words(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.nonzero(got != want)[0]
    assert not len(d), (what, f"{len(d)} of {len(want)} words differ, the first at {int(d[0])}")


def seeded_cols(seed, n_cols, log):
    """Seeded columns with the boundary words 0, 1, P - 1 in their first rows."""
    v = np.random.default_rng(seed).integers(0, P, (n_cols, 1 << log), dtype=np.uint32)
    for c in range(n_cols):
        v[c, :min(3, 1 << log)] = np.roll(np.array([0, 1, P - 1], np.uint32), c)[:min(3, 1 << log)]
    return v


# ---- 1. commit lattice ----------------------------------------------------------------------------------------------------------

class CommitColumns:
    """The host columns of the commit lattice by (log, column count): a size's columns are the same in every shape that holds it."""

    def __init__(self):
        self.cols = {}

    def get(self, log, n):
        if (log, n) not in self.cols:
            self.cols[(log, n)] = seeded_cols(7000 + 32 * log + n, n, log)
            self.cols[(log, n)].setflags(write=False)
        return self.cols[(log, n)]


@pytest.fixture(scope="module")
def commit_columns():
    c = CommitColumns()
    yield c
    c.cols.clear()


@pytest.fixture(scope="module")
def twiddles(be):
    """One twiddle tree for the whole lattice (a tree covers every smaller domain)."""
    return be.precompute_twiddles(MAX_LOG)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("A", S.LADDER)
def test_commit_lattice_roots_and_every_layer(be, oracle, commit_columns, twiddles, A, mode):
    be.set_hash_mode(mode)
    try:
        for shape in S.commit_shapes(A):
            what = (shape, "mode", mode)
            host = [commit_columns.get(log, n) for log, n in shape]
            ldes, root = oracle.lde_commit([row.copy() for arr in host for row in arr], 1, mode, threads=THREADS)
            tree_root, layers = oracle.merkle_commit(ldes, mode, want_layers=True)
            assert np.array_equal(tree_root, root), what          # the oracle's two routes agree
            # nx_commit_root: the root without the tree (reduce_to_root: node-only runs three levels at a time, cut at every injected size)
            sets = [be.columns_from_host(arr) for arr in host]
            assert np.array_equal(be.commit_root(twiddles, sets, 1), root), (what, "nx_commit_root")
            for s in sets:
                s.free()
            if len(shape) == 1:                                   # nx_lde_commit takes one size
                cols = be.columns_from_host(host[0])
                lde, lde_root = be.lde_commit(twiddles, cols, 1)
                assert np.array_equal(lde_root, root), (what, "nx_lde_commit")
                assert_same_words(lde.to_cpu(), np.stack(ldes), (what, "nx_lde_commit: extension"))
                lde.free(); cols.free()
            # nx_merkle_commit on the extended columns: every layer
            ext = []
            for arr in host:
                cols = be.columns_from_host(arr)
                ext.append(be.lde(twiddles, cols, 1))
                cols.free()
            tree = be.merkle_commit(ext)
            assert np.array_equal(tree.root(), root), (what, "nx_merkle_commit root")
            off = 0
            for k in range(A + 1, -1, -1):
                assert np.array_equal(tree.layer(k).reshape(-1), layers[off:off + (8 << k)]), (what, "layer", k)
                off += 8 << k
            del tree
            for e in ext:
                e.free()
    finally:
        be.set_hash_mode(0)


# ---- 2. proof lattice -----------------------------------------------------------------------------------------------------------

def machine_matches(be, nz, comps, kw, verify=False):
    """nx_prove_machine against machine_ref.prove_machine, every word; verify: the library's verifier accepts, and refuses a flipped word."""
    cfg = S.hip_config(nz, kw)
    ref = M.prove_machine(comps, O.default_cfg(**kw), seed=SEED, ad=AD, threads=THREADS)
    words = be.prove_machine(comps, cfg, seed=SEED, ad=AD)
    _same(ref, words, (comps, kw))
    if verify:
        claimed = be.machine_claimed_sums()
        assert nz.verify_machine(comps, cfg, words, claimed, ad=AD) is None, (comps, kw)
        bad = words.copy()
        bad[len(bad) // 2] ^= 2
        assert nz.verify_machine(comps, cfg, bad, claimed, ad=AD) is not None, (comps, kw)


@pytest.mark.parametrize("config", list(S.LADDER_CONFIGS))
@pytest.mark.parametrize("L", S.LADDER)
def test_ladder_proof_is_the_oracles_and_verifies(be, nz, oracle, L, config):
    machine_matches(be, nz, S.ladder_statement(L), S.LADDER_CONFIGS[config], verify=True)


@pytest.mark.parametrize("A,Bs", S.PAIR_GROUPS, ids=[f"{A}-{'.'.join(map(str, Bs))}" for A, Bs in S.PAIR_GROUPS])
def test_pair_proofs_are_the_oracles(be, nz, oracle, A, Bs):
    for B in Bs:
        machine_matches(be, nz, S.narrow_statement((A, B)), S.NARROW_CONFIG)


@pytest.mark.parametrize("logs", S.TRIPLES, ids=["-".join(map(str, t)) for t in S.TRIPLES])
def test_triple_proofs_are_the_oracles(be, nz, oracle, logs):
    machine_matches(be, nz, S.narrow_statement(logs), S.NARROW_CONFIG)


@pytest.mark.parametrize("variant,L", S.VARIANT_CASES, ids=[f"{v}-{L}" for v, L in S.VARIANT_CASES])
def test_ladder_proofs_under_the_configuration_variants(be, nz, oracle, variant, L):
    machine_matches(be, nz, S.ladder_statement(L), S.VARIANTS[variant])


@pytest.mark.parametrize("L", S.LADDER)
def test_synthetic_ladder_proof_is_the_oracles(be, nz, oracle, L):
    comps, ocfg = S.synth_statement(L), O.default_cfg(**S.SYNTH_CONFIG)
    words = be.prove(comps, S.hip_config(nz, S.SYNTH_CONFIG), seed=SEED, ad=AD)
    _same(oracle.prove_synth(comps, ocfg, seed=SEED, ad=AD, threads=THREADS), words, comps)
    assert oracle.verify_synth(comps, ocfg, words, ad=AD) is None


# ---- 3. session ladder ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("logs", S.SESSION_LOGS, ids=["-".join(map(str, l)) for l in S.SESSION_LOGS])
def test_session_logup_air_down_to_four_row_traces(be, nz, oracle, logs):
    """The mask wrap-around (offsets -1 / +1) on 4- and 8-row traces and the JIT composition on the smallest evaluation domains."""
    from test_gpu_parity import check_session_logup_air
    check_session_logup_air(be, nz, oracle, logs)


# ---- 4. refusals, mirrored ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def refusal_be(nz):
    """A context of its own: its live bytes are the proves' alone (no test's columns waiting for the collector)."""
    b = nz.HipBackend(0)
    yield b
    b.close()


def refused_then_usable(b, nz, refused, kw, proving):
    """`refused` gets NX_ERR_PROTOCOL "... not consumed" where the oracle throws its "fri: columns not consumed"; the context's live bytes
    are what they were, and the next prove (`proving`) on it gives the oracle's bytes."""
    cfg, ocfg = S.hip_config(nz, kw), O.default_cfg(**kw)
    ref = M.prove_machine(proving, ocfg, seed=SEED, ad=AD, threads=THREADS)
    _same(ref, b.prove_machine(proving, cfg, seed=SEED, ad=AD), ("before", proving, kw))        # also warms the context's own buffers
    with pytest.raises(RuntimeError, match=S.ORACLE_REFUSAL):
        M.prove_machine(refused, ocfg, seed=SEED, ad=AD, threads=THREADS)
    live = b.memory()[0]
    with pytest.raises(nz.NexusHipError, match=rf"error {nz.NX_ERR_PROTOCOL}: .*{S.LIBRARY_REFUSAL}"):
        b.prove_machine(refused, cfg, seed=SEED, ad=AD)
    assert b.memory()[0] == live, (refused, kw, "live bytes after the refusal")
    _same(ref, b.prove_machine(proving, cfg, seed=SEED, ad=AD), ("after", proving, kw))
    assert b.memory()[0] == live


@pytest.mark.parametrize("config", list(S.REFUSAL_CONFIGS))
@pytest.mark.parametrize("L,log_last", S.REFUSED, ids=[f"L{L}-last{ll}" for L, ll in S.REFUSED])
def test_refusal_below_the_line_leaves_the_context_clean(refusal_be, nz, oracle, L, log_last, config):
    assert nz.NX_ERR_PROTOCOL == -4
    kw = dict(S.REFUSAL_CONFIGS[config], log_last=log_last)
    refused_then_usable(refusal_be, nz, S.ladder_statement(L), kw, S.ladder_statement(log_last + 2))


def test_refusal_for_the_smallest_of_two_components(refusal_be, nz, oracle):
    """The smaller component is the one below the line: the commit phase folds its layers down to the last one before it refuses."""
    kw = dict(pow_bits=2, log_last=2)
    refused_then_usable(refusal_be, nz, S.narrow_statement((9, 3)), kw, S.narrow_statement((9, 4)))


# ---- 5. primitives --------------------------------------------------------------------------------------------------------------

def _random_points_and_alpha(oracle, seed):
    L = oracle.lib()
    ch = C.c_void_p(L.orc_channel_new())
    L.orc_channel_mix_u64(ch, seed)
    p1, p2, a = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(4, np.uint32)
    L.orc_get_random_point(ch, O.ptr(p1))
    L.orc_get_random_point(ch, O.ptr(p2))
    L.orc_channel_draw_secure_felt(ch, O.ptr(a))
    L.orc_channel_free(ch)
    return p1, p2, a


@pytest.mark.parametrize("log", [1, 2])
def test_accumulate_quotients_on_two_and_four_rows(be, oracle, log):
    """log_size 1 is quotient_small_kernel (one lane per row; no proof reaches it: an extension has at least four rows), log_size 2 one lane
    of quotient_kernel.  Two sample batches, one of them a single entry."""
    n_cols = 3
    cols = seeded_cols(8100 + log, n_cols, log)
    p1, p2, alpha = _random_points_and_alpha(oracle, 40 + log)
    rng = np.random.default_rng(log)
    b1 = [(c, rng.integers(0, P, 4, dtype=np.uint32)) for c in range(n_cols)]
    b2 = [(1, rng.integers(0, P, 4, dtype=np.uint32))]
    got = be.accumulate_quotients(be.columns_from_host(cols), alpha, [(p1, b1), (p2, b2)]).to_cpu()
    outs = [np.zeros(1 << log, np.uint32) for _ in range(4)]
    pts = np.concatenate([p1, p2])
    counts = np.array([len(b1), len(b2)], np.int32)
    cidx = np.array([c for c, _ in b1 + b2], np.int32)
    vals = np.concatenate([v for _, v in b1 + b2])
    oracle.lib().orc_accumulate_quotients(log, O.ptr_array([np.ascontiguousarray(c) for c in cols]), n_cols, O.ptr(alpha), 2, O.ptr(pts),
                                          O.ptr(counts), O.ptr(cidx), O.ptr(vals), 4, O.ptr_array(outs))
    assert_same_words(got, np.stack(outs), ("quotients", log))


def test_fri_folds_of_a_two_point_source(be, oracle):
    """src_log 1: circle_itw's L == 1 branch (fold_circle_into_line) and the line fold onto a single point."""
    L = oracle.lib()
    tw = be.precompute_twiddles(1)
    src = seeded_cols(8201, 4, 1)
    dst0 = seeded_cols(8202, 4, 0)
    _, _, alpha = _random_points_and_alpha(oracle, 51)
    d_src, d_dst = be.columns_from_host(src), be.columns_from_host(dst0)
    be.fold_circle_into_line(tw, d_dst, d_src, alpha)
    ref = [np.ascontiguousarray(c).copy() for c in dst0]
    L.orc_fold_circle_into_line(O.ptr_array(ref), O.ptr_array([np.ascontiguousarray(c) for c in src]), 1, O.ptr(alpha))
    assert_same_words(d_dst.to_cpu(), np.stack(ref), "fold_circle_into_line")
    assert not np.array_equal(np.stack(ref), dst0)
    for dbl in (0, 2):
        out = be.fold_line(tw, d_src, alpha, dbl).to_cpu()
        ref2 = [np.zeros(1, np.uint32) for _ in range(4)]
        L.orc_fold_line_dom(O.ptr_array([np.ascontiguousarray(c) for c in src]), 1, dbl, O.ptr(alpha), O.ptr_array(ref2))
        assert_same_words(out, np.stack(ref2), ("fold_line", dbl))


@pytest.mark.parametrize("log", [2, 3, 4, 9, 10])
def test_eval_at_points_below_and_at_the_table_split(be, oracle, log):
    """eval_at_point_kernel splits the index at min(log, 10) bits: below 10 the low table has fewer than 1024 entries and the high one a
    single entry (eval_tables_kernel with n < 10), at 10 the low table is full.  Two points, a polynomial sampled at both."""
    polys = seeded_cols(8300 + log, 5, log)
    p1, p2, _ = _random_points_and_alpha(oracle, 60 + log)
    idx = [0, 1, 2, 3, 4, 0, 3, 3]
    pts = [p1, p1, p1, p1, p1, p2, p2, p1]
    got = be.eval_at_points(be.columns_from_host(polys), idx, pts)
    for i, (pi, pt) in enumerate(zip(idx, pts)):
        assert np.array_equal(got[i], oracle.eval_at_point(polys[pi], pt)), (log, i)


@pytest.mark.parametrize("log", [5, 7, 8, 10, 11])
def test_transforms_at_the_sizes_between_the_tested_ones(be, oracle, log):
    """nx_interpolate_batch, nx_evaluate_batch (expand 0, 1, 2) and nx_lde_batch of 19 columns, every word."""
    n_cols = 19
    vals = seeded_cols(8400 + log, n_cols, log)
    tw = be.precompute_twiddles(log + 1)
    otw = oracle.Twiddles(log + 1)
    coeffs = np.stack([otw.interpolate(v) for v in vals])
    cols = be.columns_from_host(vals)
    be.interpolate_columns(tw, cols)
    assert_same_words(cols.to_cpu(), coeffs, (log, "interpolate"))
    for e in (0, 1, 2):
        out = be.evaluate_polynomials(tw, cols, e)
        assert_same_words(out.to_cpu(), np.stack([otw.evaluate(c, log + e) for c in coeffs]), (log, "evaluate", e))
        out.free()
    cols.free()
    cols = be.columns_from_host(vals)
    lde = be.lde(tw, cols, 1)
    assert_same_words(cols.to_cpu(), coeffs, (log, "lde: coefficients left in the columns"))
    assert_same_words(lde.to_cpu(), np.stack([otw.evaluate(c, log + 1) for c in coeffs]), (log, "lde"))
    lde.free(); cols.free()


def test_decompose_and_batch_inverse_at_2pow21(be, oracle):
    """2^21 elements: the first size at which decompose_lambda_kernel strides over more than 256 block partials (2^21 / 4096 = 512), and
    at which the grid-stride loops of the inverses and of decompose_apply_kernel make a second trip (at most n_cus * 16 blocks of 256)."""
    L = oracle.lib()
    log = 21
    src = seeded_cols(8500, 4, log)
    g, lam = be.fri_decompose(be.columns_from_host(src))
    ref = [np.zeros(1 << log, np.uint32) for _ in range(4)]
    rl = np.zeros(4, np.uint32)
    L.orc_fri_decompose(O.ptr_array([np.ascontiguousarray(c) for c in src]), log, O.ptr_array(ref), O.ptr(rl))
    assert np.array_equal(lam, rl)
    assert_same_words(g.to_cpu(), np.stack(ref), "fri_decompose")
    g.free()
    vals = np.random.default_rng(8501).integers(1, P, (1, 1 << log), dtype=np.uint32)      # non-zero, as Stwo requires
    vals[0, :2] = (1, P - 1)
    got = be.batch_inverse_m31(be.columns_from_host(vals)).to_cpu()
    want = np.zeros_like(vals)
    L.orc_batch_inverse_m31(O.ptr(np.ascontiguousarray(vals[0])), O.ptr(want[0]), C.c_size_t(1 << log))
    assert_same_words(got, want, "batch_inverse_m31")
    sec = np.random.default_rng(8502).integers(0, P, (4, 1 << log), dtype=np.uint32)
    sec[0] = np.maximum(sec[0], 1)                                                         # never the zero element
    got4 = be.batch_inverse_qm31(be.columns_from_host(sec)).to_cpu()
    want4 = [np.zeros(1 << log, np.uint32) for _ in range(4)]
    L.orc_batch_inverse_qm31(O.ptr_array([np.ascontiguousarray(c) for c in sec]), O.ptr_array(want4), C.c_size_t(1 << log))
    assert_same_words(got4, np.stack(want4), "batch_inverse_qm31")
