"""The reference side of the request structures (tests/pcs_requests.py), without a GPU: the lists are what they claim, the CPU oracle
runs every listed request, its quotients equal a plain-integer restatement of the row formula where nothing else cross-checks them
(no batch, empty batches, a repeated column, one point in two batches), the partial sums of a column-sharded quotient add up to the
whole as a fact about that formula, and the recorded grinds fall one into each launch window of nx_grind.
tests/test_gpu_pcs_requests.py then compares the device with these word for word."""
import ctypes as C

import numpy as np
import pytest

import pcs_requests as R

P = R.P


def test_the_request_lists_are_what_they_claim():
    S = R.STRUCTURES
    assert sorted(S) == ["S%d" % i for i in range(10)] and S["S0"] == []
    assert [len(cols) for _, cols in S["S8"]] == list(range(1, 10)) and len({p for p, _ in S["S8"]}) == 9
    assert all(len(set(cols)) == len(cols) for _, cols in S["S8"])                       # S8 repeats no column inside a batch
    assert [len(cols) for _, cols in S["S2"]] == [9, 0, 9] and [len(c) for _, c in S["S3"]] == [0, 9] and [len(c) for _, c in S["S4"]] == [9, 0]
    assert S["S5"] == [(0, (3, 3, 3, 3))]
    (_, perm), = S["S6"]
    assert sorted(perm) == list(range(9)) and perm != tuple(sorted(perm)) and perm != tuple(sorted(perm, reverse=True))
    (pa, ca), (pb, cb) = S["S7"]
    assert pa == pb and set(ca) != set(cb)
    assert len(S["S9"]) > 3 and len({cols for _, cols in S["S9"]}) == 1 and len({p for p, _ in S["S9"]}) == len(S["S9"])
    assert all(0 <= c < R.N_COLS for s in S.values() for _, cols in s for c in cols)
    assert all(0 <= p < R.N_POINTS for s in S.values() for p, _ in s)
    assert R.QUOT_LOGS == (1, 2, 5, 11) and (1 << 11) // 4 > 256                         # two blocks of 256 lanes at log 11
    # partial quotients: every split gives every column exactly one owner inside the world; "rank0-empty" leaves rank 0 nothing
    for world in R.WORLDS:
        for split in R.SPLITS:
            owner = R.column_owner(split, world)
            assert len(owner) == R.N_COLS and set(owner) <= set(range(world))
            assert (0 in owner) == (split != "rank0-empty")
    # evaluations: the slab case has more than one slab of ONE point, the small group comes first and sits at both ends
    sel, poly = R.slab_case()
    assert int((sel == 0).sum()) == R.SLAB + 5 > 32768 and list(np.flatnonzero(sel)) == [0, 16384, len(sel) - 1]
    big = poly[sel == 0]
    assert list(big[:5]) == [0, 1, 2, 3, 0] and list(big[R.SLAB:]) == [1, 2, 3, 0, 1]   # a second slab that read the first slab's table shows
    assert len(R.INTERLEAVED["points"]) == 7 and sorted(set(R.INTERLEAVED["points"])) == [0, 1, 2]
    assert len(set(zip(R.REPEATED["points"], R.REPEATED["poly_idx"]))) < len(R.REPEATED["points"])
    # decommit: sorted, distinct, inside the layer; one queried layer holds no column, one set leaves the big columns unqueried
    for name, queries in R.DECOMMIT_QUERIES.items():
        for log, qs in queries.items():
            assert qs == sorted(set(qs)) and 0 <= qs[0] and qs[-1] < (1 << log) and log <= max(R.DECOMMIT_LOGS), name
    assert 8 not in R.DECOMMIT_LOGS and 8 in R.DECOMMIT_QUERIES["layer-without-column"]
    assert set(R.DECOMMIT_QUERIES["small-layer-only"]) == {4}
    assert R.DECOMMIT_QUERIES["whole-layer"][4] == list(range(16))
    assert all(q ^ 1 in R.DECOMMIT_QUERIES["sibling-pairs"][9] for q in R.DECOMMIT_QUERIES["sibling-pairs"][9])


def test_the_recorded_grinds_fall_one_into_each_launch_window():
    """The file holds (seed, digest, smallest nonce) at 24 bits; nx_grind's launches cover [0, 2^24), [2^24, 2^25), [2^25, 3 2^24)."""
    cases = R.grind_cases()
    windows = R.grind_windows(R.GRIND_BITS, 3)
    assert windows == [(0, 1 << 24), (1 << 24, 1 << 25), (1 << 25, 3 << 24)]
    assert R.grind_windows(10, 3) == [(0, 1 << 16), (1 << 16, 3 << 16), (3 << 16, 7 << 16)]
    assert R.grind_windows(17, 2) == [(0, 1 << 23), (1 << 23, (1 << 23) + (1 << 24))]
    assert sorted(cases) == [1, 2, 10]
    for seed, launch in R.GRIND_LAUNCHES.items():
        digest, nonce = cases[seed]
        lo, hi = windows[launch - 1]
        assert lo <= nonce < hi, seed
        assert R.pow_zero_bits(digest, nonce) >= R.GRIND_BITS, seed
    assert cases[2][1] == 9653570 and cases[1][1] == 22921064 and cases[10][1] == 42300636


def test_the_oracle_reproduces_the_recorded_grinds(oracle):
    """Seeds 1 and 2 recomputed by the oracle's own search: 2^24.5 Blake2s hashes, this file's slowest test (several seconds).  Seed 10
    (12 s of oracle time) is held by its hash property in the test above, and its digest is recomputed here."""
    L = oracle.lib()
    cases = R.grind_cases()
    for seed in (1, 2, 10):
        ch = C.c_void_p(L.orc_channel_new())
        L.orc_channel_mix_u64(ch, seed)
        d = np.zeros(8, np.uint32)
        L.orc_channel_digest(ch, oracle.ptr(d))
        assert np.array_equal(d, cases[seed][0]), seed
        if seed != 10:
            assert L.orc_channel_grind(ch, R.GRIND_BITS) == cases[seed][1], seed
        L.orc_channel_free(ch)


def test_no_sample_point_meets_the_domain(oracle):
    """The condition of every quotient case: each denominator of each listed point is non-zero on every row."""
    for log in R.QUOT_LOGS:
        pts, _ = R.channel_points(oracle, 700 + log, R.N_POINTS)
        assert len({p.tobytes() for p in pts}) == R.N_POINTS
        for pt in pts:
            assert all(R.denominator(log, r, pt) != R.C_ZERO for r in range(1 << log)), log


def test_oracle_runs_every_quotient_request(oracle):
    for log in R.QUOT_LOGS:
        seen = set()
        for name in R.STRUCTURES:
            cols, alpha, batches = R.quotient_request(oracle, log, name)
            out = R.oracle_quotients(oracle, log, cols, alpha, batches)
            assert out.shape == (4, 1 << log) and out.max() < P
            assert (not out.any()) == (name == "S0"), (log, name)
            seen.add(out.tobytes())
        assert len(seen) == len(R.STRUCTURES)


@pytest.mark.parametrize("name", ["S0", "S2", "S5", "S7"])
@pytest.mark.parametrize("log", [1, 2])
def test_oracle_quotients_equal_the_plain_row_formula(oracle, log, name):
    cols, alpha, batches = R.quotient_request(oracle, log, name)
    want = np.array(R.model_quotients(log, cols, alpha, batches), np.uint32).reshape(-1, 4).T
    assert np.array_equal(R.oracle_quotients(oracle, log, cols, alpha, batches), want)


def test_an_empty_batch_changes_nothing_in_the_plain_formula(oracle):
    """alpha^0 = 1 and an empty numerator: [full, empty, full] is [full, full].  What S2 .. S4 rest on."""
    cols, alpha, batches = R.quotient_request(oracle, 2, "S2")
    assert R.model_quotients(2, cols, alpha, batches) == R.model_quotients(2, cols, alpha, [batches[0], batches[2]])


@pytest.mark.parametrize("world,split,line_rank", [(3, "round-robin", 1), (2, "rank0-empty", 0)])
def test_partial_sums_of_the_plain_formula_add_up(oracle, world, split, line_rank):
    """The identity tests/test_gpu_pcs_requests.py relies on, as a fact about the formula and not about the library: split the entries
    over ranks, let exactly one rank subtract the line terms of all entries, every rank advance alpha over all entries — the
    coordinate-wise sum of the parts is the whole quotient."""
    log = 2
    cols, alpha, batches = R.quotient_request(oracle, log, "S8")
    owner = R.column_owner(split, world)
    total = np.zeros((1 << log, 4), np.int64)
    for rank in range(world):
        _, _, local = R.rank_request(batches, owner, rank)
        part = np.array(R.model_quotients(log, cols, alpha, batches, local=local, include_line=rank == line_rank), np.int64)
        if not local.any() and rank != line_rank:
            assert not part.any()
        total = (total + part) % P
    assert np.array_equal(total, np.array(R.model_quotients(log, cols, alpha, batches), np.int64))
    assert np.array_equal(total.T, R.oracle_quotients(oracle, log, cols, alpha, batches))
    # and the line terms given to two ranks, or to none, do NOT add up
    twice = np.zeros_like(total)
    for rank in range(world):
        twice = (twice + np.array(R.model_quotients(log, cols, alpha, batches, local=R.rank_request(batches, owner, rank)[2], include_line=True), np.int64)) % P
    assert not np.array_equal(twice, total)


def test_rank_requests_renumber_local_columns_and_mark_the_others():
    pt, v = np.zeros(8, np.uint32), np.zeros(4, np.uint32)
    batches = [(pt, [(c, v) for c in cols]) for _, cols in R.STRUCTURES["S8"]]
    for world in R.WORLDS:
        for split in R.SPLITS:
            owner = R.column_owner(split, world)
            flags = []
            for rank in range(world):
                mine, renumbered, local = R.rank_request(batches, owner, rank)
                flat = [(c0, c1) for (_, e0), (_, e1) in zip(batches, renumbered) for (c0, _), (c1, _) in zip(e0, e1)]
                assert len(flat) == len(local) == 45
                for (c_global, c_local), is_local in zip(flat, local):
                    assert (c_local == R.NOT_LOCAL) == (not is_local) == (owner[c_global] != rank)
                    assert not is_local or mine[c_local] == c_global
                flags.append(local)
            assert np.array_equal(np.sum(flags, axis=0), np.ones(45))                    # every entry is local to exactly one rank


def test_oracle_runs_every_evaluation_request(oracle):
    for log in R.EVAL_LOGS:
        polys, pts = R.eval_request(oracle, log)
        for case in (R.INTERLEAVED, R.REPEATED):
            out = R.oracle_evals(oracle, polys, pts, case["points"], case["poly_idx"])
            assert out.shape == (len(case["points"]), 4)
            for i, (s, p) in enumerate(zip(case["points"], case["poly_idx"])):
                assert np.array_equal(out[i], oracle.eval_at_point(polys[p], pts[s]))
        if log == 0:                                                                       # a constant polynomial is its coefficient
            assert np.array_equal(R.oracle_evals(oracle, polys, pts, [0, 1], [2, 2]), [[polys[2][0], 0, 0, 0]] * 2)
    polys, pts = R.eval_request(oracle, R.SLAB_LOG)
    sel, poly = R.slab_case()
    out = R.oracle_evals(oracle, polys, pts, sel, poly)
    assert out.shape == (R.SLAB + 8, 4)
    assert len(np.unique(out, axis=0)) == 7                                                # 4 polynomials at the big point, 3 at the small one


@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_runs_every_decommit_request(oracle, mode):
    host = R.decommit_columns()
    n_at = {l: R.DECOMMIT_LOGS.count(l) for l in set(R.DECOMMIT_LOGS)}
    sizes = {}
    for name, queries in R.DECOMMIT_QUERIES.items():
        qv, hw, cw = R.oracle_decommit(oracle, host, mode, queries)
        assert len(qv) == sum(n_at.get(l, 0) * len(qs) for l, qs in queries.items()), name
        sizes[name] = (len(hw), len(cw))
    # a lone leaf needs one sibling hash per layer below the root; two sibling pairs need none at their own layer and none where their
    # paths meet (nodes 3 and 150 of layer 8 stay apart down to layer 2, their ancestors at layer 1 are siblings)
    assert sizes["one-query"][0] == 9
    assert sizes["sibling-pairs"][0] == 2 * 7
    # every node of layer 4 is rebuilt from its two children: the 32 nodes of layer 5 less the one the path from layer 9 supplies, plus
    # that path's siblings at layers 9 .. 6; nothing above layer 4
    assert sizes["whole-layer"][0] == 31 + 4
    # two nodes of layer 4: their four children, then siblings at layers 4, 3 and 2; their ancestors at layer 1 are siblings
    assert sizes["small-layer-only"][0] == 4 + 3 * 2
    # a path that starts at layer 4 never visits the larger columns; one that passes a layer with columns does
    assert sizes["small-layer-only"][1] == 0 and sizes["layer-without-column"][1] > 0
