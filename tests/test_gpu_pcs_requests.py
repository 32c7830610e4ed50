"""The per-op PCS calls by the structure of the request (-m gpu): the lists of tests/pcs_requests.py through nx_accumulate_quotients,
nx_accumulate_quotients_partial, nx_eval_at_points, nx_grind, nx_gather and nx_merkle_decommit, word for word against the CPU oracle
(tests/test_pcs_requests_cpu.py pins the lists and the oracle's side).  What no other test reaches: a request without a batch, empty
batches, repeated and permuted columns, the partial call of a column-sharded prove, the second slab of 32768 polynomials of one point,
interleaved points, the second and third launch of the proof-of-work search, gathers by themselves, decommitments of sibling pairs,
whole layers and layers without a column."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before libnexus_hip.so: whichever HIP runtime is loaded first serves the whole process)

import oracle_lib as O
import pcs_requests as R

pytestmark = pytest.mark.gpu
P = R.P
SENTINEL = 0xDEADBEEF                        # not a field element: a word the library left alone is recognisable
NX_ERR_OOM = -3                              # include/nexus_hip.h


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


@functools.lru_cache(maxsize=None)
def quotient_case(log, name):
    """(columns, alpha, batches, the oracle's quotient) — computed once, shared by the full and the partial tests, never written."""
    cols, alpha, batches = R.quotient_request(O, log, name)
    want = R.oracle_quotients(O, log, cols, alpha, batches)
    want.setflags(write=False)
    return cols, alpha, batches, want


def sentinel_columns(be, n_cols, log):
    return be.columns_from_host(np.full((n_cols, 1 << log), SENTINEL, np.uint32))


# ---- 1. quotient requests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.STRUCTURES))
@pytest.mark.parametrize("log", R.QUOT_LOGS)
def test_quotient_request_structures_match_oracle(be, oracle, log, name):
    cols, alpha, batches, want = quotient_case(log, name)
    got = be.accumulate_quotients(be.columns_from_host(cols), alpha, batches).to_cpu()
    assert np.array_equal(got, want), (log, name)
    if name == "S0":
        assert not got.any()


# ---- 2. partial quotients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", R.WORLDS)
@pytest.mark.parametrize("name", R.PARTIAL_STATEMENTS)
@pytest.mark.parametrize("log", R.PARTIAL_LOGS)
def test_partial_quotients_of_every_split_sum_to_the_whole(be, oracle, log, name, world):
    """nx_accumulate_quotients_partial on `world` ranks of one context: each rank holds its own columns only, numbers its entries'
    columns in its own order and marks the others 0xFFFFFFFF; exactly one rank adds the line terms.  The sum of the ranks' outputs mod P
    — taken on the host and, with nx_m31_add_into, on the device — is the oracle's quotient; a rank with no local entry and no line
    terms writes zeros."""
    cols, alpha, batches, want = quotient_case(log, name)
    n = 4 << log
    for split in R.SPLITS:
        owner = R.column_owner(split, world)
        requests = [R.rank_request(batches, owner, rank) for rank in range(world)]
        held = [be.columns_from_host(cols[mine]) if mine else None for mine, _, _ in requests]
        for line_rank in range(world):
            outs = []
            for rank, (mine, renumbered, local) in enumerate(requests):
                out = sentinel_columns(be, 4, log)
                be.accumulate_quotients_partial(held[rank], log, alpha, renumbered, local, rank == line_rank, out=out)
                outs.append(out)
                if not local.any() and rank != line_rank:
                    assert not out.to_cpu().any(), (split, line_rank, rank)
            host_sum = np.zeros((4, 1 << log), np.uint64)
            for out in outs:
                host_sum = (host_sum + out.to_cpu()) % P
            assert np.array_equal(host_sum.astype(np.uint32), want), (split, line_rank)
            for out in outs[1:]:
                be._chk(be.L.nx_m31_add_into(be.ctx, outs[0].ptr, out.ptr, C.c_size_t(n)))
            assert np.array_equal(outs[0].to_cpu(), want), (split, line_rank)
        if split == "rank0-empty":
            assert held[0] is None and not requests[0][2].any()


@pytest.mark.parametrize("name", R.PARTIAL_STATEMENTS)
@pytest.mark.parametrize("log", R.PARTIAL_LOGS)
def test_partial_quotients_with_every_entry_local_are_the_full_call(be, oracle, log, name):
    cols, alpha, batches, want = quotient_case(log, name)
    d = be.columns_from_host(cols)
    full = be.accumulate_quotients(d, alpha, batches).to_cpu()
    n_entries = sum(len(e) for _, e in batches)
    for local in (np.ones(n_entries, np.uint8), None):
        got = be.accumulate_quotients_partial(d, log, alpha, batches, local, True, out=sentinel_columns(be, 4, log)).to_cpu()
        assert np.array_equal(got, full) and np.array_equal(got, want), (log, name)


# ---- 3. evaluation requests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", R.EVAL_LOGS)
def test_eval_request_structures_match_oracle(be, oracle, log):
    polys, pts = R.eval_request(oracle, log)
    d = be.columns_from_host(polys)
    # no evaluation: OK, and the output is not touched
    out = np.full(8, SENTINEL, np.uint32)
    idx, p8 = np.zeros(1, np.uint32), np.ascontiguousarray(pts[0])
    be._chk(be.L.nx_eval_at_points(be.ctx, d.col_ptrs(), log, idx.ctypes.data_as(C.c_void_p), p8.ctypes.data_as(C.c_void_p), 0,
                                   out.ctypes.data_as(C.c_void_p)))
    assert (out == SENTINEL).all()
    for case in (R.INTERLEAVED, R.REPEATED):
        want = R.oracle_evals(oracle, polys, pts, case["points"], case["poly_idx"])
        got = be.eval_at_points(d, case["poly_idx"], [pts[s] for s in case["points"]])
        assert np.array_equal(got, want), (log, case)


def test_eval_second_slab_of_one_point_matches_oracle(be, oracle):
    """32768 + 5 evaluations of one point: two launches of eval_at_point_kernel, the second on the pointer table and the partial sums
    from entry 32768 on; 3 evaluations of another point at both ends and in the middle, so the large group is the SECOND one and every
    result finds its place through the group's own list."""
    polys, pts = R.eval_request(oracle, R.SLAB_LOG)
    sel, poly = R.slab_case()
    want = R.oracle_evals(oracle, polys, pts, sel, poly)
    got = be.eval_at_points(be.columns_from_host(polys), poly, np.stack(pts)[sel])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(bad), bad[:8])


# ---- 4. grind beyond the first launch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sorted(R.GRIND_LAUNCHES, key=R.GRIND_LAUNCHES.get))
def test_grind_finds_the_smallest_nonce_in_a_later_launch(be, seed):
    """24 bits: launches of 2^24 nonces; the recorded smallest nonce lies in the first (seed 2, the control), second (seed 1) and third
    (seed 10) of them.  The oracle's search is not run here (tests/test_pcs_requests_cpu.py pins the file)."""
    digest, nonce = R.grind_cases()[seed]
    lo, hi = R.grind_windows(R.GRIND_BITS, 3)[R.GRIND_LAUNCHES[seed] - 1]
    got = be.grind(digest, R.GRIND_BITS)
    assert got == nonce and lo <= got < hi
    assert R.pow_zero_bits(digest, got) >= R.GRIND_BITS


# ---- 5. gather ------------------------------------------------------------------------------------------------------------------------
def gather(be, ptrs, index):
    n = len(ptrs)
    arr = (C.c_void_p * max(1, n))(*ptrs)
    idx = np.ascontiguousarray(index, dtype=np.uint64)
    out = np.full(max(1, n), SENTINEL, np.uint32)
    be._chk(be.L.nx_gather(be.ctx, arr, idx.ctypes.data_as(C.c_void_p), C.c_size_t(n), out.ctypes.data_as(C.c_void_p)))
    return out[:n]


def test_gather_requests_match_numpy_indexing(be):
    host = [R.rand_cols(5000 + i, 1, log)[0] for i, log in enumerate(R.GATHER_LOGS)]
    dev = [be.columns_from_host(h) for h in host]
    rng = np.random.default_rng(55)

    def check(reads):
        got = gather(be, [dev[c].ptr.value for c, _ in reads], [i for _, i in reads])
        assert np.array_equal(got, np.array([host[c][i] for c, i in reads], np.uint32)), reads[:8]

    be._chk(be.L.nx_gather(be.ctx, None, None, C.c_size_t(0), None))                      # n == 0: nothing is read, not even the arguments
    check([(1, 11)])
    check([(int(c), int(rng.integers(0, len(host[c])))) for c in rng.integers(0, 3, 257)])       # two blocks
    check([(2, 777)] * 300)                                                                # one (pointer, index) pair 300 times
    check([(c, i) for c in range(3) for i in (0, len(host[c]) - 1)])                        # the first and the last word of each column
    check([(0, int(i)) for i in rng.permutation(1 << 10)])


def test_gather_reaches_the_end_of_a_one_gibibyte_column(be):
    """Index 2^28 - 1 of a 2^28-word column: a byte offset of 2^30 - 4, which no narrower index arithmetic reaches."""
    n = 1 << R.BIG_LOG
    p = C.c_void_p()
    rc = be.L.nx_alloc(be.ctx, C.c_size_t(n), C.byref(p))
    if rc == NX_ERR_OOM:
        pytest.skip("nx_alloc answered NX_ERR_OOM for the 1 GiB column")
    be._chk(rc)
    try:
        be._chk(be.L.nx_memset_zero(be.ctx, p, C.c_size_t(n)))
        words = {0: 0x11111111, n // 2: 0x22222222, n - 1: 0x33333333, n - 2: 0x44444444}
        for i, w in words.items():
            v = np.array([w], np.uint32)
            be._chk(be.L.nx_upload(be.ctx, C.c_void_p(p.value + 4 * i), v.ctypes.data_as(C.c_void_p), C.c_size_t(1)))
        index = [0, n // 2, n - 1, n - 2, 1, n // 2 - 1, n // 2 + 1, n - 3]
        got = gather(be, [p.value] * len(index), index)
        assert list(got) == [words.get(i, 0) for i in index]
    finally:
        be.L.nx_free(be.ctx, p)


# ---- 6. decommit requests ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1])
def committed(request, be):
    """The mixed tree, committed once per hash mode."""
    host = R.decommit_columns()
    be.set_hash_mode(request.param)
    try:
        sets = [be.columns_from_host(h) for h in host]
        tree = be.merkle_commit(sets)
        be.sync()
    finally:
        be.set_hash_mode(0)
    return request.param, host, sets, tree


@pytest.mark.parametrize("name", list(R.DECOMMIT_QUERIES))
def test_decommit_request_structures_match_oracle(be, oracle, committed, name):
    mode, host, sets, tree = committed
    queries = R.DECOMMIT_QUERIES[name]
    r_qv, r_hw, r_cw = R.oracle_decommit(oracle, host, mode, queries)
    be.set_hash_mode(mode)
    try:
        qv, hw, cw = be.merkle_decommit(tree, sets, queries)
    finally:
        be.set_hash_mode(0)
    assert len(qv) == len(r_qv) and np.array_equal(qv, r_qv)
    assert len(hw) == len(r_hw) and np.array_equal(hw, r_hw)
    assert len(cw) == len(r_cw) and np.array_equal(cw, r_cw)
