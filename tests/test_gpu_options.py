"""The context options' promise on the device (-m gpu): "None of them changes a result: proofs, roots and transforms are bit-identical
under every setting" (include/nexus_hip.h), for the kernel-shape switches no other file flips.  Everything is bit-exact against the
CPU oracle; every test that sets an option uses a context of its own and closes it.

A. every pass plan of plan13 (csrc/fft13.hip) reachable at 2^14 .. 2^18 points by lowering "fft.kmax", at the smallest size that
   produces it, through nx_interpolate_batch, nx_evaluate_batch (expand 0, 1, 2) and nx_lde_batch (blow-up 2: fft13_lde with 2 .. 6
   passes); K = 10 and K = 11 (the run-time-K kernels fft13_kernel<..., 0> and lde_mid_kernel<4, 0>) at 2^23 / 2^24 points, the
   smallest sizes that hold such a pass, and K = 7 at 2^20; "fft.fused" = 0.
B. whole proofs of one machine statement that crosses every threshold involved, under each switch.
C. merkle_pair_levels_kernel next to injected columns, every layer.
D. the untiled finalize_last scan above the tiled one's threshold."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import machine_ref as M
import oracle_lib as O

pytestmark = pytest.mark.gpu
P = O.P
THREADS = max(4, min(16, os.cpu_count() or 4))
T13 = 13   # layers of the first pass (csrc/fft13.hip T13_S)


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


def backend_with(nz, options):
    """A context of its own under `options` ({name: value}); the caller closes it."""
    b = nz.HipBackend(0)
    for name, value in options.items():
        b.set_option(name, value)
        assert b.get_option(name) == value
    return b


# ---- A. pass plans --------------------------------------------------------------------------------------------------------------

def plan13(n, kmax):
    """csrc/fft13.hip plan13 restated: the layer counts of the passes above the first 13 layers of a 2^n-point transform."""
    rest = n - T13
    nhi = -(-rest // kmax)
    return [rest // nhi + (1 if i < rest % nhi else 0) for i in range(nhi)]


# (log, kmax, K list): the smallest (log, then kmax) that produces each K list reachable at 2^14 .. 2^18 points
SMALL_PLANS = [
    (14, 1, [1]), (15, 2, [2]), (16, 3, [3]), (17, 4, [4]), (18, 5, [5]),
    (15, 1, [1, 1]), (16, 2, [2, 1]), (17, 2, [2, 2]), (18, 3, [3, 2]),
    (16, 1, [1, 1, 1]), (18, 2, [2, 2, 1]),
    (17, 1, [1, 1, 1, 1]),
    (18, 1, [1, 1, 1, 1, 1]),
]
# One column each, (log, kmax, K list, expands).  K = 10 and 11 are the run-time-K instantiations (launch13_k / launch_mid `default:`);
# K <= n - 13, so 2^23 / 2^24 points are the smallest sizes with such a pass.  The 2^26-point evaluation of the 2^24 case is left out:
# its oracle side alone (a 2^25-entry twiddle tree and the transform) is more than ten seconds of host time.  K = 7 (2^20 points, the
# default kmax) is the one layer count below 10 that no default plan of the plain transforms and no row above reaches.
SINGLE_COLUMN_PLANS = [(20, 9, [7], (0, 1, 2)), (23, 10, [10], (0, 1, 2)), (24, 11, [11], (0, 1))]


def plan_id(case):
    return f"log{case[0]}-kmax{case[1]}-K{'.'.join(map(str, case[2]))}"


def test_plan_table_covers_every_reachable_plan():
    """The tables above against the planner's rule: every case yields the K list it claims, and the small table holds EVERY distinct K
    list of 2^14 .. 2^18 points under kmax 1 .. 11 — a planner change makes this fail instead of letting the sweep test less."""
    for log, kmax, ks in SMALL_PLANS + [c[:3] for c in SINGLE_COLUMN_PLANS]:
        assert plan13(log, kmax) == ks, (log, kmax)
        assert sum(ks) == log - T13 and max(ks) <= kmax
    reachable = {tuple(plan13(log, kmax)) for log in range(14, 19) for kmax in range(1, 12)}
    assert reachable == {tuple(ks) for _, _, ks in SMALL_PLANS}
    assert len(SMALL_PLANS) == len(reachable) == 13
    for log, kmax, ks in SMALL_PLANS:   # each at its smallest size
        assert not any(tuple(plan13(l, k)) == tuple(ks) for l in range(14, log) for k in range(1, 12)), (log, kmax)
    # the generic kernels: a pass of 10 / 11 layers needs 2^23 / 2^24 points
    assert all(max(plan13(l, k)) < 10 for l in range(14, 23) for k in range(1, 12))
    assert all(max(plan13(23, k)) < 11 for k in range(1, 12))


def seeded_cols(seed, n_cols, log):
    """Seeded columns with the boundary words 0, 1, P - 1 in their first rows."""
    v = np.random.default_rng(seed).integers(0, P, (n_cols, 1 << log), dtype=np.uint32)
    for c in range(n_cols):
        v[c, :3] = np.roll(np.array([0, 1, P - 1], np.uint32), c)
    return v


class TransformRefs:
    """The oracle's side of the transform sweeps, computed once per (log, column count) and handed out read-only."""

    def __init__(self, oracle):
        self.oracle, self.tw, self.refs = oracle, {}, {}

    def twiddles(self, root_log):
        """One twiddle tree per sweep (a tree of root_log covers domains up to 2^(root_log + 1); larger trees serve smaller sizes)."""
        if root_log not in self.tw:
            self.tw[root_log] = self.oracle.Twiddles(root_log)
        return self.tw[root_log]

    def get(self, log, n_cols, expands, root_log):
        key = (log, n_cols)
        if key not in self.refs:
            vals = seeded_cols(4000 + log, n_cols, log)
            otw = self.twiddles(root_log)
            coeffs = np.stack([otw.interpolate(v) for v in vals])
            vals.setflags(write=False); coeffs.setflags(write=False)
            self.refs[key] = (vals, coeffs, {})
        vals, coeffs, evals = self.refs[key]
        for e in expands:
            if e not in evals:
                evals[e] = np.stack([self.twiddles(root_log).evaluate(c, log + e) for c in coeffs])
                evals[e].setflags(write=False)
        return vals, coeffs, evals

    def drop(self, log, n_cols):
        self.refs.pop((log, n_cols), None)


@pytest.fixture(scope="module")
def refs(oracle):
    r = TransformRefs(oracle)
    yield r
    r.refs.clear(); r.tw.clear()


def assert_same_words(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.nonzero(got != want)[0]
    assert not len(d), (what, f"{len(d)} of {len(want)} words differ, the first at {int(d[0])}")


def check_three_routes(b, refs, log, n_cols, expands, root_log, what):
    """nx_interpolate_batch, nx_evaluate_batch at every expand and nx_lde_batch (blow-up 2) of the same columns, every word."""
    vals, coeffs, evals = refs.get(log, n_cols, expands, root_log)
    tw = b.precompute_twiddles(log + 1)          # domains up to 2^(log + 2)
    cols = b.columns_from_host(vals)
    b.interpolate_columns(tw, cols)
    assert_same_words(cols.to_cpu(), coeffs, (what, "interpolate"))
    for e in expands:
        out = b.evaluate_polynomials(tw, cols, e)      # e > 0: the top pass replicates the coefficient tiles (rep_log = e)
        got = out.to_cpu()
        out.free()
        assert_same_words(got, evals[e], (what, "evaluate", e))
        del got
    cols.free()
    cols = b.columns_from_host(vals)
    lde = b.lde(tw, cols, 1)
    assert_same_words(cols.to_cpu(), coeffs, (what, "lde: coefficients left in the columns"))
    assert_same_words(lde.to_cpu(), evals[1], (what, "lde"))
    lde.free(); cols.free()


@pytest.mark.parametrize("log,kmax,ks", SMALL_PLANS, ids=[plan_id(c) for c in SMALL_PLANS])
def test_every_pass_plan_matches_oracle(nz, refs, log, kmax, ks):
    """Non-first passes of K layers with runs of 2^(13 - K) words, 1 .. 5 of them: three columns (an odd count) through the three
    transform routes.  The fused LDE runs its inverse passes before lde_mid_kernel and its forward passes after it with P = 2 .. 6."""
    assert plan13(log, kmax) == ks
    b = nz.HipBackend(0)
    try:
        b.set_option("fft.kmax", kmax)
        check_three_routes(b, refs, log, 3, (0, 1, 2), 19, (log, kmax, ks))
    finally:
        b.close()


@pytest.mark.parametrize("log,kmax,ks,expands", SINGLE_COLUMN_PLANS, ids=[plan_id(c) for c in SINGLE_COLUMN_PLANS])
def test_passes_of_7_10_and_11_layers_match_oracle(nz, refs, log, kmax, ks, expands):
    """K = 10 and 11: fft13_kernel<INV, false, 1, 4, 0> (forward and inverse) and lde_mid_kernel<4, 0>, the instantiations that read the
    layer count from the pass descriptor and that only "fft.kmax" above 9 reaches; K = 7: fft13_kernel<..., 7>.  One column, every
    word of every route; the three cases share one oracle twiddle tree."""
    assert plan13(log, kmax) == ks
    b = nz.HipBackend(0)
    try:
        b.set_option("fft.kmax", kmax)
        check_three_routes(b, refs, log, 1, expands, 24, (log, kmax, ks))
    finally:
        b.close()
        refs.drop(log, 1)     # up to hundreds of megabytes of reference nobody else reads


@pytest.mark.parametrize("log", [14, 16])
def test_unfused_lde_matches_oracle_and_the_fused_launch(be, nz, refs, log):
    """"fft.fused" = 0: nx_lde_batch as separate inverse and forward passes — the oracle's words, which are also the fused launch's."""
    vals, coeffs, evals = refs.get(log, 3, (1,), 19)
    got = {}
    b = nz.HipBackend(0)
    try:
        b.set_option("fft.fused", 0)
        for name, x in (("unfused", b), ("fused", be)):
            assert x.get_option("fft.fused") == (name == "fused")
            tw = x.precompute_twiddles(log)
            cols = x.columns_from_host(vals)
            lde = x.lde(tw, cols, 1)
            got[name] = (cols.to_cpu(), lde.to_cpu())
            lde.free(); cols.free()
    finally:
        b.close()
    for name in ("unfused", "fused"):
        assert_same_words(got[name][0], coeffs, (log, name, "coefficients"))
        assert_same_words(got[name][1], evals[1], (log, name, "lde"))
    assert np.array_equal(got["unfused"][1], got["fused"][1])


# ---- B. whole proofs ------------------------------------------------------------------------------------------------------------

# 2^16 rows: the fused LDE (>= 2^14), the tiled scan (>= 2^13), trees of >= 2^17 leaves (under the default "merkle.top" 7 / "merkle.subtree" 14
# merkle_pair_levels_kernel pairs levels from 16 up, where no column is injected: the composition and FRI-layer trees here; the trace
# trees, with the second component's columns at level 15, under "merkle.top" 1 / "merkle.subtree" 0) and 70 main columns (with
# "fft.batch_cols" = 1 a launch takes 64 columns of 2^16 rows: two batches for the side streams; with 256 one)
STATEMENT = [(16, 4, 70, 16), (14, 3, 17, 8, 2), (9, 2, 6, 4, 1)]
CONFIGS = {
    "std": dict(pow_bits=4, log_constraint_degree=2),
    "raw0-alpha-first": dict(pow_bits=4, log_constraint_degree=2, hash_mode=1, fri_alpha_mode=1),
}
SEED, AD = 21, b"options"
SETTINGS = {
    "kmax-1": {"fft.kmax": 1},
    "kmax-2": {"fft.kmax": 2},
    "kmax-11": {"fft.kmax": 11},
    "unfused-lde": {"fft.fused": 0},
    "batch-1-streams-1": {"fft.batch_cols": 1, "fft.streams": 1},
    "batch-1-streams-4": {"fft.batch_cols": 1, "fft.streams": 4},
    "batch-256-streams-1": {"fft.batch_cols": 256, "fft.streams": 1},
    "batch-256-streams-4": {"fft.batch_cols": 256, "fft.streams": 4},
    "no-pair-levels": {"merkle.pair_levels": 0},
    "pair-levels-from-13": {"merkle.pair_levels": 1, "merkle.top": 1, "merkle.subtree": 0},
    "host-channel": {"fri.device_channel": 0},
    "host-channel-no-tail": {"fri.device_channel": 0, "fri.tail": 0},
    "untiled-scan": {"logup.scan_tiled": 0},
    "all-off": {"fft.fused": 0, "merkle.pair_levels": 0, "fri.device_channel": 0, "fri.tail": 0, "logup.scan_tiled": 0},
}
PROOF_CASES = [("std", s) for s in SETTINGS] + [("raw0-alpha-first", "pair-levels-from-13"), ("raw0-alpha-first", "host-channel-no-tail")]


@pytest.fixture(scope="module")
def oracle_proofs(oracle):
    """The oracle's proof of STATEMENT per protocol configuration, proved once."""
    cache = {}

    def get(config):
        if config not in cache:
            cache[config] = M.prove_machine(STATEMENT, O.default_cfg(**CONFIGS[config]), seed=SEED, ad=AD, threads=THREADS)
            cache[config].setflags(write=False)
        return cache[config]
    return get


@pytest.mark.parametrize("config,setting", PROOF_CASES, ids=[f"{c}-{s}" for c, s in PROOF_CASES])
def test_proof_is_the_oracles_under_every_switch(nz, oracle_proofs, config, setting):
    """nx_prove_machine of STATEMENT in a context of its own under one setting of the switches: every proof word is the oracle's."""
    ref = oracle_proofs(config)
    b = backend_with(nz, SETTINGS[setting])
    try:
        words = b.prove_machine(STATEMENT, nz.default_config(**CONFIGS[config]), seed=SEED, ad=AD)
    finally:
        b.close()
    assert_same_words(words, ref, (config, SETTINGS[setting], "proof words; the roots are words 6..37"))


# ---- C. pair levels next to injected columns ------------------------------------------------------------------------------------

# In each triple the second tree injects a column exactly at the upper level of what would be a pair (log - 1 of the build loop:
# the pair must not be taken), the third one a level lower (the pair is taken and the column goes into the next layer)
PAIR_TREES = [
    ([17, 17, 17], [{}, {"merkle.pair_levels": 0}]),
    ([17, 17, 15], [{}, {"merkle.pair_levels": 0}]),
    ([17, 17, 14], [{}, {"merkle.pair_levels": 0}]),
    ([14, 14], [{"merkle.top": 1, "merkle.subtree": 0}]),
    ([14, 12], [{"merkle.top": 1, "merkle.subtree": 0}]),
    ([14, 11], [{"merkle.top": 1, "merkle.subtree": 0}]),
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("logs,option_sets", PAIR_TREES, ids=["-".join(map(str, t[0])) for t in PAIR_TREES])
def test_pair_levels_beside_injected_columns_every_layer(nz, oracle, logs, option_sets, mode):
    host = [np.random.default_rng(5000 + 10 * sum(logs) + i).integers(0, P, 1 << l, dtype=np.uint32) for i, l in enumerate(logs)]
    root, layers = oracle.merkle_commit(host, mode, want_layers=True)
    for options in option_sets:
        b = backend_with(nz, options)
        try:
            assert b.get_option("merkle.pair_levels") == options.get("merkle.pair_levels", 1)
            b.set_hash_mode(mode)
            sets = [b.columns_from_host(h) for h in host]
            tree = b.merkle_commit(sets)
            assert np.array_equal(tree.root(), root), (logs, mode, options)
            off = 0
            for k in range(max(logs), -1, -1):
                assert np.array_equal(tree.layer(k).reshape(-1), layers[off:off + (8 << k)]), (logs, mode, options, "layer", k)
                off += 8 << k
            del tree, sets
        finally:
            b.close()


# ---- D. the untiled scan above the tiled one's threshold ------------------------------------------------------------------------

@pytest.mark.parametrize("log,k", [(13, 2), (17, 3)])
def test_untiled_finalize_last_matches_oracle_from_2pow13_up(nz, oracle, log, k):
    """"logup.scan_tiled" = 0: the per-row scan kernels at the sizes the tiled ones normally take (one 4096-row scan block has two
    blocks at 2^13 rows, 32 at 2^17), as test_logup_finalize_last_batch_matches_oracle compares the default."""
    rng = np.random.default_rng(log * 10 + k)
    cols = [rng.integers(0, P, (4, 1 << log), dtype=np.uint32) for _ in range(k)]
    b = nz.HipBackend(0)
    try:
        b.set_option("logup.scan_tiled", 0)
        dev = [b.columns_from_host(c) for c in cols]
        claimed = b.logup_finalize_last_batch(dev)
        got = [d.to_cpu() for d in dev]
        del dev
    finally:
        b.close()
    for c, g, cs in zip(cols, got, claimed):
        ref_cols, ref_sum = oracle.logup_finalize_last([x.copy() for x in c])
        assert np.array_equal(cs, ref_sum) and np.array_equal(g, np.stack(ref_cols))
