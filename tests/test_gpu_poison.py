"""Every entry on dirty memory.  The context options "debug.poison" (1, 2, 3: 0xA5A5A5A5, 0xFFFFFFFF, 0x00000001) and "debug.poison_free"
make the caching allocator fill every block it hands out, fresh or recycled, and every block it takes back: a temporary that is read
before all of it was written, or a block that is still in use when it is freed, no longer finds zero pages or a previous call's
plausible field elements.  tests/poison_sites.py is the audit of the allocation sites; this file is the sweep — the cases and judges of
the other GPU test modules, run on a poisoned context under each pattern.  Every comparison is against the CPU oracle, a Python model or
numpy, never against an unpoisoned device run.

a. the facility itself (nx_alloc / nx_free / nx_ctx_memory);  b. every case of placement.CASES at shift 0;  c. the entries that table
does not hold;  d. whole proofs, word for word: nx_prove_synth, nx_prove_machine, the host-trace entries, the session (nx_prover_create
.. nx_prover_prove) with a device logup program, two and four trace trees, nx_prover_tree_commit_host, a shared and adopted
preprocessed tree (nx_prover_tree_share / nx_prover_tree_adopt), the size-dependent paths, and A, B, A on one context;  e. one statement on two thread-ranks (nx_comm_local_create)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import machine_ref as M
import oracle_lib as O
import placement as PL
import test_gpu_access_chain as T_CHAIN
import test_gpu_machine as T_MACHINE
import test_gpu_multiplicities_sparse as T_SPARSE
import test_gpu_parity as T_PARITY
import test_gpu_pcs_requests as T_REQ
import test_gpu_placement as T_PLACE
import test_gpu_trace_check as T_CHECK
import test_gpu_trace_partition as T_PART
import test_verifier_cpu as V

pytestmark = pytest.mark.gpu
P = O.P
THREADS = max(4, min(16, os.cpu_count() or 4))
WORD = {1: 0xA5A5A5A5, 2: 0xFFFFFFFF, 3: 0x00000001}
PATTERNS = sorted(WORD)
SWEEP_CASES = [c for c in PL.CASES if c.shift == 0 and c.refuse is None]


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


def poisoned(nz, pattern):
    b = nz.HipBackend(0)
    b.set_option("debug.poison", pattern)
    b.set_option("debug.poison_free", 1)
    assert b.get_option("debug.poison") == pattern and b.get_option("debug.poison_free") == 1
    return b


@pytest.fixture(scope="module", params=PATTERNS, ids=["a5a5a5a5", "ffffffff", "00000001"])
def be(request, nz):
    """one context per pattern, dressed as the fixtures of the modules whose runners it is handed to"""
    b = poisoned(nz, request.param)
    b.pattern = request.param
    b.tw = b.precompute_twiddles(PL.TW_LOG)
    b.kernels = {}
    yield b
    for k in b.kernels.values():
        k.close()
    b.tw = None
    b.close()


@pytest.fixture(scope="module")
def ap():
    import nexus_zkvm_amd.air_program as ap
    return ap


def device_errors_end_the_run(nz, what, fn, *args):
    """as test_gpu_placement.check: after the first HIP error nothing more is launched on this device by this run"""
    try:
        return fn(*args)
    except nz.NexusHipError as e:
        if "HIP error" in str(e):
            pytest.exit(f"{what}: {e}", returncode=3)
        raise


def same(ref, words, what):
    assert len(ref) == len(words), (what, len(ref), len(words))
    if not np.array_equal(ref, words):
        pytest.fail(f"{what}: first differing proof word {int(np.nonzero(np.asarray(ref) != np.asarray(words))[0][0])} of {len(ref)}")


# ---------------------------------------------------------------------------------------------------------------- a. the facility

def _alloc(b, n_words):
    p = C.c_void_p()
    b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(n_words), C.byref(p)))
    return p


def _words(b, p, n_words):
    out = np.empty(n_words, np.uint32)
    b.sync()
    b._chk(b.L.nx_download(b.ctx, out.ctypes.data_as(C.c_void_p), p, C.c_size_t(n_words)))
    return out


def _facility_calls(b, pattern):
    """the calls of the facility test; pattern 0: the same calls on a context that does not poison"""
    seen = []
    for n in (64, 4096, 1 << 16):
        p = _alloc(b, n)
        if pattern:
            assert (_words(b, p, n) == WORD[pattern]).all(), ("a fresh block", n)
        data = np.arange(1, n + 1, dtype=np.uint32)
        b._chk(b.L.nx_upload(b.ctx, p, data.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        assert np.array_equal(_words(b, p, n), data)
        b._chk(b.L.nx_free(b.ctx, p))
        if pattern:
            b.set_option("debug.poison", 0)                   # the block comes back as dev_free left it
        q = _alloc(b, n)
        if pattern:
            b.set_option("debug.poison", pattern)
        assert q.value == p.value, "the free list is keyed by the exact rounded size: the block just freed comes back"
        if pattern:
            got = _words(b, q, n)
            assert (got == WORD[pattern]).all(), ("a freed block", n, got[:4])
        seen.append(b.memory())
        r = _alloc(b, n)                                       # a second, recycled-or-fresh block while the first is live
        if pattern:
            assert (_words(b, r, n) == WORD[pattern]).all()
        seen.append(b.memory())
        b._chk(b.L.nx_free(b.ctx, r))
        b._chk(b.L.nx_free(b.ctx, q))
        seen.append(b.memory())
    return seen


@pytest.mark.parametrize("pattern", PATTERNS)
def test_blocks_come_filled_go_filled_and_the_accounting_does_not_move(nz, pattern):
    b, plain = poisoned(nz, pattern), nz.HipBackend(0)
    try:
        assert plain.get_option("debug.poison") == 0 and plain.get_option("debug.poison_free") == 0
        assert _facility_calls(b, pattern) == _facility_calls(plain, 0), "nx_ctx_memory: live and peak bytes"
        with pytest.raises(nz.NexusHipError):
            b.set_option("debug.poison", 4)
    finally:
        b.close(); plain.close()


def test_poison_free_alone_does_nothing(nz):
    b = nz.HipBackend(0)
    try:
        b.set_option("debug.poison_free", 1)
        n = 4096
        p = _alloc(b, n)
        data = np.arange(7, n + 7, dtype=np.uint32)
        b._chk(b.L.nx_upload(b.ctx, p, data.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        b._chk(b.L.nx_free(b.ctx, p))
        q = _alloc(b, n)
        assert q.value == p.value and np.array_equal(_words(b, q, n), data)
        b._chk(b.L.nx_free(b.ctx, q))
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------- b. the placement table

_PLANS = {}
_build = PL.build


def _plan_once(case):
    if case not in _PLANS:
        _PLANS[case] = _build(case)
    return _PLANS[case]


@pytest.fixture(autouse=True)
def _plans_are_built_once(monkeypatch):
    """the oracle side of a case is the expensive half: one plan serves the three contexts"""
    monkeypatch.setattr(PL, "build", _plan_once)


def test_the_sweep_is_the_whole_table_at_shift_0():
    assert len(SWEEP_CASES) == 322 and {c.entry for c in SWEEP_CASES} == set(PL.TABLE) and len(PL.TABLE) == 44
    assert set(T_PLACE.RUN) == set(PL.TABLE)


@pytest.mark.parametrize("family", PL.FAMILIES)
def test_every_placement_case_on_poisoned_blocks(be, nz, oracle, family):
    cases = [c for c in SWEEP_CASES if PL.TABLE[c.entry].family == family]
    assert cases
    for case in cases:
        T_PLACE.check(be, nz, case)


# ---------------------------------------------------------------------------------------------------------------- c. the other entries

def test_nx_logup_multiplicities_sparse(be, nz):
    device_errors_end_the_run(nz, "sparse multiplicities", T_SPARSE.test_key_extremes, be, [16, 16])
    device_errors_end_the_run(nz, "sparse multiplicities", T_SPARSE.test_missing_and_out_of_range_rows, be)


def test_nx_trace_access_chain(be, nz):
    device_errors_end_the_run(nz, "access chain", T_CHAIN.test_two_linear_streams_through_both_entries, be, nz, 2)
    device_errors_end_the_run(nz, "access chain", T_CHAIN.test_one_key_chained_by_add, be, nz, 1025)


def test_nx_trace_partition_create_and_fill_with_every_step(be, nz):
    """nx_trace_partition_create, then nx_trace_partition_fill whose destinations take NX_PART_ALL beside the classes (make_dests)"""
    for n_steps, n_classes in ((257, 3), (1025, 40)):
        device_errors_end_the_run(nz, "trace partition", T_PART.test_exact_against_the_model, be, nz, n_steps, n_classes)


def test_nx_gather(be, nz):
    device_errors_end_the_run(nz, "nx_gather", T_REQ.test_gather_requests_match_numpy_indexing, be)


def test_nx_grind(be, nz, oracle):
    """the recorded launches of tests/golden/grind_launches.json, and the oracle's own search at small difficulties"""
    for seed in sorted(T_REQ.R.GRIND_LAUNCHES, key=T_REQ.R.GRIND_LAUNCHES.get):
        device_errors_end_the_run(nz, "nx_grind", T_REQ.test_grind_finds_the_smallest_nonce_in_a_later_launch, be, seed)
    device_errors_end_the_run(nz, "nx_grind", T_PARITY.test_grind_matches_oracle, be, oracle)


@pytest.mark.parametrize("mode", [0, 1])
def test_nx_merkle_decommit_layer_and_root(be, nz, oracle, mode):
    """nx_merkle_decommit in both hash modes; nx_merkle_layer / nx_merkle_root: every layer and the root of a mixed tree against the oracle's"""
    device_errors_end_the_run(nz, "nx_merkle_decommit", T_PARITY.test_merkle_decommit_matches_oracle, be, oracle, mode)
    case = next(c for c in SWEEP_CASES if c.entry == "nx_merkle_commit" and c.log == 5 and c.variant == ("mixed-raw0" if mode else "mixed"))
    device_errors_end_the_run(nz, "nx_merkle_layer", T_PLACE.check, be, nz, case)        # tree_words: MerkleTree.layer of every level, MerkleTree.root


def test_nx_air_check_and_nx_prover_check(be, nz, ap):
    """a passing trace, and failing ones: the constraint and the row the device names are the CPU model's (check_against_interpreter)"""
    run = lambda fn, *a: device_errors_end_the_run(nz, "trace check", fn, be, nz, *a)      # noqa: E731
    run(T_CHECK.test_valid_logup_statements_pass, dict(logs=(5, 7)))
    run(T_CHECK.test_valid_synthetic_machine_passes_with_any_tree_count, ap, 2)
    run(T_CHECK.test_one_cell_of_a_main_column)
    run(T_CHECK.test_offsets_beyond_one, ap, 17)
    run(T_CHECK.test_the_primitive_on_uncommitted_columns_gives_the_session_report)       # nx_air_check


def test_nx_synth_fill_tree(be, nz, oracle):
    comps = [(7, 3, 21, 6), (5, 2, 4, 3)]
    for tree in range(3):
        got = device_errors_end_the_run(nz, "nx_synth_fill_tree", lambda: [c for s in be.synth_fill_tree(comps, tree, 5, inter_seed=99) for c in s.to_cpu()])
        want = oracle.synth_tree_columns(comps, tree, 5, inter_seed=99)
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), tree


def test_nx_generate_secure_powers(be):
    felt = np.array([5, P - 1, 123456789, 2], np.uint32)
    got = be.generate_secure_powers(felt, 6)
    want, acc = [], (1, 0, 0, 0)
    for _ in range(6):
        want.append(acc)
        acc = _qm31_mul(acc, tuple(int(x) for x in felt))
    assert np.array_equal(np.asarray(got, np.uint32).reshape(-1, 4), np.array(want, np.uint32))


def _cm31_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _qm31_mul(x, y):
    """(a + b u)(c + d u) with u^2 = 2 + i over CM31 = M31[i]"""
    a, b, c, d = x[:2], x[2:], y[:2], y[2:]
    ac, bd = _cm31_mul(a, c), _cm31_mul(b, d)
    r = _cm31_mul(bd, (2, 1))
    ad, bc = _cm31_mul(a, d), _cm31_mul(b, c)
    return ((ac[0] + r[0]) % P, (ac[1] + r[1]) % P, (ad[0] + bc[0]) % P, (ad[1] + bc[1]) % P)


# ---------------------------------------------------------------------------------------------------------------- d. whole proofs

SYNTH_KW = dict(pow_bits=6)
STATEMENTS = [(comps, kw, 7, V.AD) for comps, kw in V.MACHINE] + [V.SWEEP_MACHINE]
LOG12_FUSED = ([(12, 3, 10, 4)], dict(pow_bits=4), 3, b"fused")
LOG12_STREAMS = ([(12, 4, 20, 8), (9, 2, 5, 4)], dict(pow_bits=4), 4, b"streams")


@pytest.fixture(scope="module")
def refs(oracle):
    """the oracle's proofs, each proved once"""
    cache = {}

    def machine(i):
        comps, kw, seed, ad = STATEMENTS[i] if isinstance(i, int) else i
        key = (repr(comps), repr(sorted(kw.items())), seed, ad)
        if key not in cache:
            cache[key] = M.prove_machine(comps, O.default_cfg(**kw), seed=seed, ad=ad, threads=THREADS)
            cache[key].setflags(write=False)
        return cache[key]

    def synth():
        if "synth" not in cache:
            cache["synth"] = oracle.prove_synth(V.SYNTH, O.default_cfg(**SYNTH_KW), seed=3, ad=V.AD)
        return cache["synth"]
    machine.synth = synth
    return machine


def test_nx_prove_synth_and_nx_prove_machine(be, nz, refs):
    run = lambda fn, *a, **k: device_errors_end_the_run(nz, "prove", lambda: fn(*a, **k))      # noqa: E731
    same(refs.synth(), run(be.prove, V.SYNTH, nz.default_config(**SYNTH_KW), seed=3, ad=V.AD), "nx_prove_synth")
    for i, (comps, kw, seed, ad) in enumerate(STATEMENTS):
        same(refs(i), run(be.prove_machine, comps, nz.default_config(**kw), seed=seed, ad=ad), ("nx_prove_machine", i))


def test_a_then_b_then_a_on_one_context(be, nz, refs):
    """two shapes in turn: B's blocks are cut from what A freed, A's second proof from what B freed"""
    for i in (0, 3, 0):
        comps, kw, seed, ad = STATEMENTS[i]
        same(refs(i), device_errors_end_the_run(nz, "prove", lambda: be.prove_machine(comps, nz.default_config(**kw), seed=seed, ad=ad)), ("A, B, A", i))


def test_nx_prove_machine_host_and_host_narrow(be, nz, refs):
    """HostFeed's hand-ordered slots: the trace comes from host memory in both orders, and with its flag columns one byte wide"""
    idx = {}
    for i, (comps, kw, seed, ad) in enumerate(STATEMENTS):
        cfg = nz.default_config(**kw)

        def go():
            pre = [c for s in be.synth_fill_tree(comps, 0, seed) for c in s.to_cpu()]
            main = [c for s in be.synth_fill_tree(comps, 1, seed) for c in s.to_cpu()]
            same(refs(i), be.prove_machine_host(comps, cfg, pre, main, ad=ad), ("nx_prove_machine_host", i))
            n = len(pre[0])
            if n not in idx:
                idx[n] = O.finalize_column(np.arange(n, dtype=np.uint32))

            def natural(col):
                nat = np.zeros(len(col), np.uint32)
                if len(col) not in idx:
                    idx[len(col)] = O.finalize_column(np.arange(len(col), dtype=np.uint32))
                nat[idx[len(col)]] = col
                return nat
            same(refs(i), be.prove_machine_host(comps, cfg, [natural(c) for c in pre], [natural(c) for c in main], ad=ad, coset_order=True), ("coset order", i))
            flags = [k < 2 for c in comps for k in range(c[1])]              # is_first / is_last of every component
            assert all(pre[j].max() <= 1 for j, f in enumerate(flags) if f)
            pre8 = [c.astype(np.uint8) if f else c for c, f in zip(pre, flags)]
            same(refs(i), be.prove_machine_host_narrow(comps, cfg, pre8, main, ad=ad), ("nx_prove_machine_host_narrow", i))
            same(refs(i), be.prove_machine_host_narrow(comps, cfg, pre, main, ad=ad, pre_as=[np.uint8 if f else None for f in flags]), ("packed on the host", i))
        device_errors_end_the_run(nz, "host prove", go)


def test_the_session_with_a_device_logup_program(be, nz, oracle):
    """nx_logup_program and nx_logup_col / nx_logup_finalize_last write straight into the columns nx_prover_tree_begin hands out"""
    device_errors_end_the_run(nz, "session", T_PARITY.test_session_with_the_interaction_trace_generated_from_the_recorded_air, be, nz, oracle)
    device_errors_end_the_run(nz, "session", T_PARITY.test_session_end_to_end_with_device_logup, be, nz, oracle, 6)


@pytest.mark.parametrize("n_trees", [2, 4])
def test_the_session_with_two_and_four_trace_trees(be, nz, oracle, n_trees):
    device_errors_end_the_run(nz, "session", T_PARITY.test_session_with_two_and_four_trace_trees, be, nz, oracle, n_trees)


def test_the_session_with_nx_prover_tree_commit_host(be, nz, oracle):
    device_errors_end_the_run(nz, "session", T_MACHINE.test_session_commit_from_host_columns_with_kept_evaluations, be, nz, oracle)


def test_a_preprocessed_tree_shared_and_adopted_whoever_goes_first(be, nz, oracle, ap):
    """nx_prover_tree_share / nx_prover_tree_adopt.  The donor session is destroyed before an adopter proves (the parity test's third
    session), and the other way round: the adopter is destroyed, then the donor proves again.  A block of the shared tree that went
    back to the allocator with either session would be filled before the survivor reads it."""
    import air_examples as AE
    device_errors_end_the_run(nz, "shared tree", T_PARITY.test_preprocessed_tree_shared_between_sessions_and_proofs, be, nz, oracle)
    log, n_pre, n_main, n_inter = 8, 3, 9, 6
    kw = dict(pow_bits=3)
    cfg, ocfg = nz.default_config(**kw), O.default_cfg(**kw)
    comps = [(log, n_pre, n_main, n_inter)]
    comp = AE.synthetic_component(ap, log, n_pre, n_main, n_inter)
    pre = oracle.synth_tree_columns(comps, 0, 1)

    def statement(session, seed, first_tree):
        session.mix_u64(log)
        first_tree(session)
        session.commit(oracle.synth_tree_columns(comps, 1, seed))
        session.mix_felts(np.zeros(4, np.uint32))
        session.commit(oracle.synth_tree_columns(comps, 2, seed, inter_seed=5))
        return session.prove([comp])

    want = {seed: statement(O.ProverSession(ocfg, log), seed, lambda s: s.commit(pre)) for seed in (21, 22)}

    def go():
        donor = be.prover_session(cfg, log)
        same(want[21], statement(donor, 21, lambda s: s.commit(pre)), "donor")
        shared = donor.share_tree(0)
        adopter = be.prover_session(cfg, log)
        same(want[22], statement(adopter, 22, lambda s: s.adopt_tree(shared)), "adopter")
        adopter.close()
        shared.release()
        churn = _alloc(be, 3 << log)                          # the allocator hands out and takes back blocks in between
        be._chk(be.L.nx_free(be.ctx, churn))
        same(want[21], donor.prove([comp]), "donor, after the adopter has gone")
        donor.close()
    device_errors_end_the_run(nz, "shared tree", go)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_fused_tree_launch_at_2pow12(nz, refs, pattern):
    """"merkle.fused" lowered to 12 (default 21): the composition tree and the FRI layers of a 2^12-row statement take tree_alloc + the fused launch"""
    comps, kw, seed, ad = LOG12_FUSED
    b = poisoned(nz, pattern)
    try:
        b.set_option("merkle.fused", 12)
        same(refs(LOG12_FUSED), device_errors_end_the_run(nz, "fused", lambda: b.prove_machine(comps, nz.default_config(**kw), seed=seed, ad=ad)), "merkle.fused = 12")
    finally:
        b.close()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_side_streams_at_2pow12(nz, refs, pattern):
    """one column per batch on four streams: the transforms of neighbouring columns run on the side streams while blocks come and go on the main one"""
    comps, kw, seed, ad = LOG12_STREAMS
    b = poisoned(nz, pattern)
    try:
        b.set_option("fft.streams", 4)
        b.set_option("fft.batch_cols", 1)
        same(refs(LOG12_STREAMS), device_errors_end_the_run(nz, "streams", lambda: b.prove_machine(comps, nz.default_config(**kw), seed=seed, ad=ad)), "fft.streams = 4")
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------- e. two thread-ranks

@pytest.mark.parametrize("pattern", PATTERNS)
def test_one_statement_on_two_thread_ranks(nz, refs, monkeypatch, pattern):
    """nx_comm_local_create: each rank's context is poisoned (the NX_DEBUG_POISON* variables seed the contexts the ranks create); the
    proof of every rank is the oracle's.  The ranks are threads with a context each on device 0, as everywhere in test_gpu_machine.py, so a
    box with one device runs this too: nothing is skipped."""
    monkeypatch.setenv("NX_DEBUG_POISON", str(pattern))
    monkeypatch.setenv("NX_DEBUG_POISON_FREE", "1")
    monkeypatch.setenv("NX_FRI_DIST_MIN_LOG", "0")
    comps, kw, seed, ad = STATEMENTS[1]
    cfg = nz.default_config(**kw)

    def rank(b, comm, r):
        assert b.get_option("debug.poison") == pattern and b.get_option("debug.poison_free") == 1
        return b.prove_machine(comps, cfg, seed=seed, ad=ad, comm=comm)
    for words in T_MACHINE._run_ranks(nz, 2, rank):
        same(refs(1), words, "two thread-ranks")
