"""The out-of-memory path, without exhausting the card.  The context option "debug.fail_alloc" = k refuses the k-th request the block
allocator sees, on the host, before any driver call; "debug.alloc_count" says how many requests a call makes.  Every test below refuses
EVERY request of its statement in turn and requires what the header promises after NX_ERR_OOM: the injection's text, the live count of
nx_ctx_memory back at its value, NULL handles, the option back at 0, and — after the sweep, and for the session after every single
refusal — the oracle's words from the same context.  "mem.limit_bytes" and "mem.cache_bytes" are run at the measured peak of a statement
and one rounding unit below it.  tests/oom_sites.py is the audit of the allocation sites.

1. the sweep over every statement;  2. the same under "debug.poison" + "debug.poison_free" for the session and the machine proofs;
3. the budget;  4. the cache cap;  5. a refusal on one of two thread-ranks: nobody waits out "comm.timeout_ms";  6. option plumbing.

Longest single call of test 5 observed on an MI355X: 3 ms of the 5000 ms timeout (asserted below against half the timeout)."""
import ctypes as C
import gc
import os
import threading
import time

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import access_chain_model as CM
import keccak_memcheck_model as KMM
import keccak_round_model as KRM
import machine_ref as MR
import oom_sites as OOM
import oracle_lib as O
import placement as PL
import test_gpu_access_chain as T_CHAIN
import test_gpu_keccak_memcheck as T_KMEM
import test_gpu_keccak_round as T_KROUND
import test_gpu_multiplicities as T_MULT
import test_gpu_multiplicities_sparse as T_SPARSE
import test_gpu_placement as T_PLACE
import test_gpu_prev_access as T_PREV
import test_gpu_trace_partition as T_PART

pytestmark = pytest.mark.gpu
NX_OK, NX_ERR_ARG, NX_ERR_OOM = 0, -2, -3
P = O.P
THREADS = max(4, min(16, os.cpu_count() or 4))
ROUND = 256                                     # the allocator's rounding of a request

# the machine statement: a v1-shaped component and a table component (its fractions read preprocessed evaluations: the keep list of tree 0)
MACHINE = [(6, 4, 10, 8), (6, 4, 3, 4, 0, MR.TABLE)]
MACHINE_KW, MACHINE_SEED, MACHINE_AD = dict(pow_bits=3), 7, b"oom"
# the session statement: two recorded components of 2^6 and 2^4 rows over three trees
SESSION = [(6, 3, 9, 6), (4, 2, 4, 3)]
SESSION_KW, SESSION_SEED, SESSION_INTER = dict(pow_bits=3), 21, 5


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def ap():
    import nexus_zkvm_amd.air_program as ap
    return ap


def _dressed(b):
    """as the fixtures of the modules whose runners the context is handed to"""
    b.tw = b.precompute_twiddles(PL.TW_LOG)
    b.kernels = {}
    return b


def _undress(b):
    for k in b.kernels.values():
        k.close()
    b.tw = None
    b.close()


@pytest.fixture(scope="module")
def be(nz):
    b = _dressed(nz.HipBackend(0))
    yield b
    _undress(b)


@pytest.fixture(scope="module", params=[0, 1], ids=["plain", "poisoned"])
def pbe(request, nz, be):
    """the context of tests 1 and 2: the plain one, and one whose blocks come and go filled with 0xA5A5A5A5"""
    if not request.param:
        yield be
        return
    b = nz.HipBackend(0)
    b.set_option("debug.poison", 1)
    b.set_option("debug.poison_free", 1)
    yield b
    b.close()


# ---------------------------------------------------------------------------------------------------------------- the oracle, once

@pytest.fixture(scope="module")
def machine_ref_words(oracle):
    w = MR.prove_machine(MACHINE, O.default_cfg(**MACHINE_KW), seed=MACHINE_SEED, ad=MACHINE_AD, threads=THREADS)
    w.setflags(write=False)
    return w


@pytest.fixture(scope="module")
def session_inputs(oracle, ap):
    """(trees as host columns, components, the oracle session's proof words)"""
    import air_examples as AE
    trees = [oracle.synth_tree_columns(SESSION, 0, SESSION_SEED), oracle.synth_tree_columns(SESSION, 1, SESSION_SEED),
             oracle.synth_tree_columns(SESSION, 2, SESSION_SEED, inter_seed=SESSION_INTER)]
    comps, at = [], [0, 0, 0]
    for log, n_pre, n_main, n_inter in SESSION:
        comps.append(AE.synthetic_component(ap, log, n_pre, n_main, n_inter, pre0=at[0], main0=at[1], inter0=at[2]))
        at = [at[0] + n_pre, at[1] + n_main, at[2] + n_inter]
    so = oracle.ProverSession(O.default_cfg(**SESSION_KW), SESSION[0][0])
    so.mix_u64(len(SESSION))
    so.commit(trees[0]); so.commit(trees[1])
    so.mix_felts(np.zeros(4, np.uint32))
    so.commit(trees[2])
    words = so.prove(comps)
    words.setflags(write=False)
    return trees, comps, words


# ---------------------------------------------------------------------------------------------------------------- the machinery

def _live(b, want=None):
    """the allocator's live count; device columns of a refused run go back with their Python owners, so where the count is not the wanted
    one it is read again after a collection (a collection per call costs more than the calls of a sweep)"""
    live = b.memory()[0]
    if want is None or live != want:
        gc.collect()
        live = b.memory()[0]
    return live


def _call(nz, fn):
    """(None, result) or (the error's text, None)"""
    try:
        return None, fn()
    except nz.NexusHipError as e:
        text = str(e)
    if "HIP error" in text:                      # a device error: nothing more is launched on this device by this run
        pytest.exit(text, returncode=3)
    return text, None


def _is_injection(text, k):
    return f"error {NX_ERR_OOM}:" in text and f"debug.fail_alloc: request {k} (" in text and text.rstrip().endswith("bytes) refused")


def same(ref, words, what):
    assert words is not None and len(ref) == len(words), (what, len(ref), None if words is None else len(words))
    if not np.array_equal(ref, words):
        pytest.fail(f"{what}: first differing word {int(np.nonzero(np.asarray(ref) != np.asarray(words))[0][0])} of {len(ref)}")


def sweep(b, nz, entry, run, judge, repeats=None):
    """run(): the statement, one call after the other, raising NexusHipError where the library refuses; judge(result) compares a result
    with the oracle's.  Every request of a clean run is refused in turn.  repeats: a statement that checks a refused call on the spot and
    makes it again (SessionRun) hands in the function that says which refusal it met last; it must end in the oracle's words.
    Returns (positions, tolerated)."""
    judge(run())                                 # warm: kernels compiled, nothing of the count depends on the cache
    live0, c0 = _live(b), b.get_option("debug.alloc_count")
    judge(run())
    n = b.get_option("debug.alloc_count") - c0
    assert n >= 1 and _live(b) == live0, (entry, n)
    tolerated = 0
    for k in range(1, n + 1):
        b.set_option("debug.fail_alloc", k)
        text, got = _call(nz, run)
        assert b.get_option("debug.fail_alloc") == 0, (entry, k, "the statement made fewer requests than its clean run")
        if repeats:
            assert text is None and _is_injection(repeats(), k), (entry, k, text, repeats())
            judge(got)
        elif text is None:                       # the refusal was absorbed: only where the audit says so, and with the same words
            assert entry in OOM.TOLERATING_ENTRIES, (entry, k, "NX_OK after a refused request, and no row of tests/oom_sites.py tolerates it")
            judge(got)
            tolerated += 1
        else:
            assert _is_injection(text, k), (entry, k, text)
        got = None
        assert _live(b, live0) == live0, (entry, k, "blocks of the refused call are still live")
    judge(run())                                 # the context is as usable as before
    assert _live(b) == live0
    return n, tolerated


# ---------------------------------------------------------------------------------------------------------------- the statements

def _machine_host_columns(b):
    pre = [c for s in b.synth_fill_tree(MACHINE, 0, MACHINE_SEED) for c in s.to_cpu()]
    main = [c for s in b.synth_fill_tree(MACHINE, 1, MACHINE_SEED) for c in s.to_cpu()]
    return pre, main


class SessionRun:
    """The session statement call by call.  A refused call is checked on the spot — live count, NULL handles — and then REPEATED: the
    statement goes on from the state the refusal left (the transcript untouched, the tree no longer begun, the channel restored), so the
    words at its end are the oracle's for every position of the refusal."""

    def __init__(self, b, nz, inputs):
        self.b, self.nz, (self.trees, self.comps, _) = b, nz, inputs
        self.refusals = []

    def step(self, what, fn, after_refusal=None):
        live = self.b.memory()[0]
        try:
            return fn()
        except self.nz.NexusHipError as e:
            text = str(e)
            if "debug.fail_alloc: request" not in text:      # not the injection (a budget, a device error): the statement ends here
                raise
        self.refusals.append((what, text))
        assert f"error {NX_ERR_OOM}:" in text, (what, text)
        if after_refusal:
            after_refusal()
        assert _live(self.b, live) == live, (what, "blocks of the refused call are still live")
        return fn()                              # the option is back at 0: the same call, the words it always returns

    def commit_device(self, ss, cols):
        """nx_prover_tree_begin, nx_upload, nx_prover_tree_commit"""
        b, logs = self.b, O.u32([int(np.log2(len(c))) for c in cols])
        ptrs = (C.c_void_p * len(cols))()

        def begin():
            for i in range(len(cols)):
                ptrs[i] = 0xDEAD0
            b._chk(b.L.nx_prover_tree_begin(ss.h, logs.ctypes.data_as(C.c_void_p), len(logs), ptrs))

        def begin_and_commit():
            self.step("nx_prover_tree_begin", begin, lambda: self.all_null(ptrs, len(cols)))
            for c, d in zip(cols, ptrs):
                b._chk(b.L.nx_upload(b.ctx, C.c_void_p(d), c.ctypes.data_as(C.c_void_p), C.c_size_t(len(c))))
            ss.tree_commit()
        digest = ss.digest()
        # a refused commit leaves the tree not begun and the transcript as it was: begin it again, fill it again, commit it
        self.step("nx_prover_tree_commit", begin_and_commit, lambda: self.untouched(ss, digest))

    @staticmethod
    def all_null(ptrs, n):
        assert all(not ptrs[i] for i in range(n)), "nx_prover_tree_begin left a column pointer behind its refusal"

    @staticmethod
    def untouched(ss, digest):
        assert np.array_equal(ss.digest(), digest), "a refused commit changed the transcript"

    def commit_host_narrow(self, ss, cols, narrow, keep):
        """nx_prover_tree_commit_host_narrow with a keep list; the kept columns are the caller's blocks, taken before the tree is begun"""
        b, nz = self.b, self.nz
        arrs, kinds = nz._narrow_columns([c.astype(np.uint8) if f else c for c, f in zip(cols, narrow)])
        logs = O.u32([int(np.log2(len(c))) for c in cols])
        kept = {}
        for k in keep:
            kept[k] = self.step("nx_alloc", lambda k=k: nz.DeviceColumns(b, 1, int(logs[k])))
        ki = O.u32(list(kept))
        kd = (C.c_void_p * len(kept))(*[d.ptr.value for d in kept.values()])
        ptrs = (C.c_void_p * len(cols))()
        root = np.zeros(8, np.uint32)

        def begin_and_commit():
            self.step("nx_prover_tree_begin", lambda: b._chk(b.L.nx_prover_tree_begin(ss.h, logs.ctypes.data_as(C.c_void_p), len(logs), ptrs)), lambda: self.all_null(ptrs, len(cols)))
            b._chk(b.L.nx_prover_tree_commit_host_narrow(ss.h, *nz._host_columns(arrs, kinds), 0, ki.ctypes.data_as(C.c_void_p), len(kept), kd, root.ctypes.data_as(C.c_void_p)))
        digest = ss.digest()
        self.step("nx_prover_tree_commit_host_narrow", begin_and_commit, lambda: self.untouched(ss, digest))
        for k, d in kept.items():
            assert np.array_equal(d.to_cpu()[0], cols[k]), ("kept evaluations of column", k)
        return kept

    def __call__(self):
        b, nz = self.b, self.nz
        cfg = nz.default_config(**SESSION_KW)
        h = C.c_void_p(0xDEAD0)

        def create():
            h.value = 0xDEAD0
            b._chk(b.L.nx_prover_create(b.ctx, C.byref(cfg), SESSION[0][0], C.byref(h)))

        def null_handle():
            assert not h.value, "nx_prover_create left a handle behind its refusal"
        self.step("nx_prover_create", create, null_handle)
        ss = nz.ProverSession.__new__(nz.ProverSession)
        ss.be, ss.cfg, ss.h = b, cfg, h
        try:
            ss.mix_u64(len(SESSION))
            flags = [k < 2 for c in SESSION for k in range(c[1])]                  # is_first / is_last of every component: one byte wide
            kept = self.commit_host_narrow(ss, self.trees[0], flags, keep=(0, len(self.trees[0]) - 1))
            self.commit_device(ss, self.trees[1])
            ss.mix_felts(np.zeros(4, np.uint32))
            self.commit_device(ss, self.trees[2])
            digest = ss.digest()
            words = self.step("nx_prover_prove", lambda: ss.prove(self.comps), lambda: self.untouched(ss, digest))
            kept.clear()
            return words
        finally:
            ss.close()


def _trace_statements(b, nz):
    """{entry: run} of the statements that check themselves against their models (the runners of their own test modules)"""
    case = lambda entry, log, variant="": PL.Case(entry, log, 0, variant, None)      # noqa: E731
    placed = lambda c: (lambda: T_PLACE.run_case(b, nz, c))                          # noqa: E731

    def prev_access():
        rng = np.random.default_rng(501)
        streams = [T_PREV.make_stream(rng, [8, 5], 5, 2, flags=bool(s)) for s in range(2)]
        T_PREV.run(b, nz, streams, [8, 5], 2, [3, P - 1], cap=64)

    def access_chain():
        rng = np.random.default_rng(502)
        streams = [CM.column_stream(rng, [8, 5], 5, 2, rng.integers(0, 40, 32), flags=bool(s), epoch=0 if s == 0 else 1, linear=s == 0) for s in range(2)]
        streams.append(CM.block_stream(rng, [8, 5], np.array([1, 7, 30], np.uint32), 4, 2, rng.integers(0, 37, 3), rule=[CM.ADD, CM.GIVEN], delta=[1, 0], epoch=1))
        T_CHAIN.run(b, nz, streams, [8, 5], 2, [0, 9], cap=64)

    def partition():
        rng = np.random.default_rng(503)
        T_PART.run(b, nz, T_PART.classes(rng, 40, 3, with_none=True), 3, T_PART.make_sources(rng, 40))

    def keccak_round():
        states = KRM.test_states(3, seed=6)
        want = KRM.fill(states, 0, 4, 6)
        main, pre, out, _ = T_KROUND.run(b, nz, states, 0, 4, 6)
        T_KROUND._same(main, want["main"], "main"); T_KROUND._same(pre, want["pre"], "preprocessed")
        assert np.array_equal(out, want["out"])

    def keccak_memcheck():
        k = next(i for i, s in enumerate(KMM.SHAPES) if s[1] == 3)
        want = KMM.want(k)
        main, pre, out, _ = T_KMEM.run(b, nz, *KMM.inputs(k), KMM.SHAPES[k][0])
        T_KROUND._same(main, want["main"], "main"); T_KROUND._same(pre, want["pre"], "preprocessed")
        assert np.array_equal(out, want["out"])

    return {
        "nx_commit_root": placed(case("nx_commit_root", 5)),                         # columns of 2^5, 2^3 and 2^1 rows
        "nx_lde_commit": placed(case("nx_lde_commit", 6)),
        "nx_merkle_commit": placed(case("nx_merkle_commit", 5, "mixed")),
        "nx_logup_program": placed(case("nx_logup_program", 6)),
        "nx_logup_multiplicities": lambda: T_MULT.test_weights(b, [8]),
        "nx_logup_multiplicities_sparse": lambda: T_SPARSE.test_key_extremes(b, [16, 16]),
        "nx_trace_prev_access": prev_access,
        "nx_trace_access_chain": access_chain,
        "nx_trace_partition_create": partition,                                      # and nx_trace_partition_fill, through the handle
        "nx_trace_keccak_round": keccak_round,
        "nx_trace_keccak_memory_check": keccak_memcheck,
    }


TRACE_ENTRIES = ("nx_commit_root", "nx_lde_commit", "nx_merkle_commit", "nx_logup_program", "nx_logup_multiplicities", "nx_logup_multiplicities_sparse", "nx_trace_prev_access",
                 "nx_trace_access_chain", "nx_trace_partition_create", "nx_trace_keccak_round", "nx_trace_keccak_memory_check")


# ---------------------------------------------------------------------------------------------------------------- 1, 2. the sweep

def test_the_session_statement_at_every_position(pbe, nz, session_inputs):
    """tests 1 and 2 for the session: nx_prover_create, a host-fed narrow tree with a keep list, two device trees, nx_prover_prove.
    SessionRun repeats the refused call, so every position ends in the oracle's words."""
    ref = session_inputs[2]
    runs = []

    def run():
        r = SessionRun(pbe, nz, session_inputs)
        runs.append(r)
        return r()
    last = lambda: runs[-1].refusals[0][1] if len(runs[-1].refusals) == 1 else repr(runs[-1].refusals)      # noqa: E731
    n, tolerated = sweep(pbe, nz, "nx_prover_prove", run, lambda w: same(ref, w, "session"), repeats=last)
    refused = [r.refusals for r in runs[2:2 + n]]
    assert all(len(r) == 1 for r in refused) and tolerated == 0 and not runs[0].refusals and not runs[1].refusals and not runs[-1].refusals
    assert {w for r in refused for w, _ in r} == {"nx_prover_create", "nx_alloc", "nx_prover_tree_begin", "nx_prover_tree_commit", "nx_prover_tree_commit_host_narrow", "nx_prover_prove"}
    print(f"session statement: {n} allocator requests, {tolerated} tolerated")


def test_nx_prove_machine_at_every_position(pbe, nz, machine_ref_words):
    cfg = nz.default_config(**MACHINE_KW)
    n, tolerated = sweep(pbe, nz, "nx_prove_machine", lambda: pbe.prove_machine(MACHINE, cfg, seed=MACHINE_SEED, ad=MACHINE_AD), lambda w: same(machine_ref_words, w, "nx_prove_machine"))
    print(f"nx_prove_machine: {n} allocator requests, {tolerated} tolerated")


def test_nx_prove_machine_host_at_every_position(pbe, nz, machine_ref_words):
    cfg = nz.default_config(**MACHINE_KW)
    pre, main = _machine_host_columns(pbe)
    n, tolerated = sweep(pbe, nz, "nx_prove_machine_host", lambda: pbe.prove_machine_host(MACHINE, cfg, pre, main, ad=MACHINE_AD), lambda w: same(machine_ref_words, w, "nx_prove_machine_host"))
    print(f"nx_prove_machine_host: {n} allocator requests, {tolerated} tolerated")


def test_nx_prover_check_at_every_position(be, nz, session_inputs):
    trees, comps, _ = session_inputs
    ss = be.prover_session(nz.default_config(**SESSION_KW), SESSION[0][0])
    try:
        ss.mix_u64(len(SESSION))
        for t in trees:
            ss.commit(t)
        digest = ss.digest()

        def run():
            report = ss.check(comps)
            assert report.ok, report
            return True
        n, tolerated = sweep(be, nz, "nx_prover_check", run, lambda ok: None)
        assert np.array_equal(ss.digest(), digest) and tolerated == 0
        print(f"nx_prover_check: {n} allocator requests")
    finally:
        ss.close()


@pytest.mark.parametrize("entry", TRACE_ENTRIES)
def test_every_other_entry_at_every_position(be, nz, oracle, entry):
    run = _trace_statements(be, nz)[entry]
    n, tolerated = sweep(be, nz, entry, run, lambda checked_by_the_runner: None)
    assert tolerated == 0
    print(f"{entry}: {n} allocator requests")


def test_handles_are_null_after_a_refusal(be, nz):
    """the *out of every entry that makes a handle or hands out a block, preset to a non-NULL word"""
    L, ctx = be.L, be.ctx
    live0 = _live(be)

    def refused(call, k=1):
        out = C.c_void_p(0xDEAD0)
        be.set_option("debug.fail_alloc", k)
        rc = call(out)
        assert rc == NX_ERR_OOM and _is_injection(f"error {rc}: " + L.nx_last_error(ctx).decode(), k), (rc, L.nx_last_error(ctx))
        assert not out.value and be.get_option("debug.fail_alloc") == 0 and _live(be) == live0
    refused(lambda out: L.nx_alloc(ctx, C.c_size_t(100), C.byref(out)))
    for k in (1, 2, 3, 4):
        refused(lambda out: L.nx_twiddles_create(ctx, 5, C.byref(out)), k)
    cols = nz.DeviceColumns(be, 3, 4).upload(np.arange(48, dtype=np.uint32).reshape(3, 16))
    live0 = _live(be)
    logs = O.u32([4, 4, 4])
    refused(lambda out: L.nx_merkle_commit(ctx, cols.col_ptrs(), logs.ctypes.data_as(C.c_void_p), 3, C.byref(out)))
    digests = nz.DeviceColumns(be, 8, 3).upload(np.arange(64, dtype=np.uint32).reshape(8, 8))
    live0 = _live(be)
    refused(lambda out: L.nx_merkle_from_leaves(ctx, digests.ptr, 3, C.byref(out)))
    cls = nz.DeviceColumns(be, 1, 6).upload((np.arange(64, dtype=np.uint32) % 3)[None, :])
    live0 = _live(be)
    counts = np.full(3, 77, np.uint32)
    for k in (1, 2):
        refused(lambda out: L.nx_trace_partition_create(ctx, cls.ptr, 40, 3, counts.ctypes.data_as(C.c_void_p), C.byref(out)), k)
    assert (counts == 77).all()
    cfg = nz.default_config(pow_bits=3)
    for k in (1, 2, 3, 4):
        refused(lambda out: L.nx_prover_create(ctx, C.byref(cfg), 5, C.byref(out)), k)


# ---------------------------------------------------------------------------------------------------------------- 3. the budget

def _budget(b, nz, run, ref, what):
    b.trim()
    live0 = _live(b)
    b.memory(reset_peak=True)
    same(ref, run(), what)
    peak = b.memory()[1]
    assert peak > live0 and peak % ROUND == 0, (live0, peak)
    # P holds the statement: with the blocks of the clean run cached, and from an empty cache
    for trimmed in (False, True):
        if trimmed:
            b.trim()
        b.set_option("mem.limit_bytes", peak)
        assert b.get_option("mem.limit_bytes") == peak
        b.memory(reset_peak=True)
        same(ref, run(), (what, "at its peak", trimmed))
        assert b.memory()[1] == peak and b.get_option("mem.cached_bytes") + _live(b) <= peak
    # P - 256 is the first budget that cannot
    for trimmed in (False, True):
        if trimmed:
            b.trim()
        b.set_option("mem.limit_bytes", peak - ROUND)
        text, got = _call(nz, run)
        assert got is None and f"error {NX_ERR_OOM}:" in text and "dev_alloc: " in text and f" live of a budget of {peak - ROUND} (mem.limit_bytes)" in text, text
        refused, live_then = int(text.split("dev_alloc: ")[1].split(" bytes refused: ")[0]), int(text.split(" bytes refused: ")[1].split(" live of")[0])
        assert refused % ROUND == 0 and live_then + refused == peak, text
        assert _live(b) == live0 and b.get_option("mem.cached_bytes") + live0 <= peak - ROUND
    b.set_option("mem.limit_bytes", 0)
    same(ref, run(), (what, "the limit lifted"))
    assert _live(b) == live0
    return peak - live0


def test_the_budget_at_the_peak_and_one_unit_below(nz, machine_ref_words, session_inputs):
    b = nz.HipBackend(0)
    try:
        cfg = nz.default_config(**MACHINE_KW)
        pm = _budget(b, nz, lambda: b.prove_machine(MACHINE, cfg, seed=MACHINE_SEED, ad=MACHINE_AD), machine_ref_words, "nx_prove_machine")
        ps = _budget(b, nz, lambda: SessionRun(b, nz, session_inputs)(), session_inputs[2], "session")
        print(f"peak above the context's own blocks: machine {pm} bytes, session {ps} bytes")
        # a limit below the live count is accepted and refuses the next request, nothing else
        p = C.c_void_p()
        b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(1024), C.byref(p)))
        live = _live(b)
        assert live >= 4096
        b.set_option("mem.limit_bytes", ROUND)
        assert _live(b) == live
        q = C.c_void_p(0xDEAD0)
        assert b.L.nx_alloc(b.ctx, C.c_size_t(16), C.byref(q)) == NX_ERR_OOM and not q.value
        assert f"dev_alloc: 256 bytes refused: {live} live of a budget of 256 (mem.limit_bytes)" in b.L.nx_last_error(b.ctx).decode()
        b._chk(b.L.nx_free(b.ctx, p))                  # giving back is never refused
        b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(16), C.byref(q)))      # 64 bytes round to the whole budget
        assert q.value and b.L.nx_alloc(b.ctx, C.c_size_t(16), C.byref(p)) == NX_ERR_OOM
        b.set_option("mem.limit_bytes", 0)
        b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(16), C.byref(p)))
        b._chk(b.L.nx_free(b.ctx, p)); b._chk(b.L.nx_free(b.ctx, q))
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the cache cap

@pytest.mark.parametrize("cap", [0, 4 << SESSION[0][0]], ids=["nothing", "one-column"])
def test_the_cache_never_holds_more_than_its_cap(nz, machine_ref_words, session_inputs, cap):
    b = nz.HipBackend(0)
    try:
        assert b.get_option("mem.cache_bytes") == 192 << 30
        cfg = nz.default_config(**MACHINE_KW)
        same(machine_ref_words, b.prove_machine(MACHINE, cfg, seed=MACHINE_SEED, ad=MACHINE_AD), "default cap")
        assert b.get_option("mem.cached_bytes") > cap
        b.set_option("mem.cache_bytes", cap)
        assert b.get_option("mem.cache_bytes") == cap and b.get_option("mem.cached_bytes") <= cap, "what is held beyond the new cap goes back at once"
        seen = []

        class Watched(SessionRun):
            def step(self, what, fn, after_refusal=None):
                out = SessionRun.step(self, what, fn, after_refusal)
                seen.append(self.b.get_option("mem.cached_bytes"))
                return out
        same(session_inputs[2], Watched(b, nz, session_inputs)(), "session")
        same(machine_ref_words, b.prove_machine(MACHINE, cfg, seed=MACHINE_SEED, ad=MACHINE_AD), "nx_prove_machine")
        seen.append(b.get_option("mem.cached_bytes"))
        p = C.c_void_p()
        b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(1 << 12), C.byref(p)))
        b._chk(b.L.nx_free(b.ctx, p))                  # 16 KiB: over either cap
        seen.append(b.get_option("mem.cached_bytes"))
        assert len(seen) > 8 and max(seen) <= cap, seen
        if cap:
            b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(cap // 4), C.byref(p)))
            b._chk(b.L.nx_free(b.ctx, p))
            assert b.get_option("mem.cached_bytes") == cap, "a block of exactly the cap is kept"
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. two thread-ranks

SHARDED_TIMEOUT_MS = 5000


def test_a_refusal_on_one_rank_at_every_position_and_nobody_waits(be, nz, machine_ref_words):
    """the machine statement on 2 thread-ranks; rank 1 is refused at EVERY position of its clean run — the positions before its first
    collective (nx_twiddles_create, the slabs and kept buffers of stage_tree) are the ones that used to leave rank 0 in the vote's
    all-gather until "comm.timeout_ms".  Both ranks return, each call in well under half the timeout, the group is broken, and after
    nx_comm_group_reset the same group proves the single-GPU words."""
    world = 2
    cfg = nz.default_config(**MACHINE_KW)
    group = nz.LocalGroup(world)
    bes = [nz.HipBackend(0) for _ in range(world)]
    comms = [bes[r].local_comm(group, r) for r in range(world)]
    for b in bes:
        b.set_option("comm.timeout_ms", SHARDED_TIMEOUT_MS)
        b.set_option("fri.dist_min_log", 0)

    def on_ranks():
        out = [None] * world

        def run(r):
            out[r] = _call(nz, lambda: bes[r].prove_machine(MACHINE, cfg, seed=MACHINE_SEED, ad=MACHINE_AD, comm=comms[r]))
        th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
        t0 = time.monotonic()
        for x in th:
            x.start()
        for x in th:
            x.join(timeout=4 * SHARDED_TIMEOUT_MS / 1000)
        assert not any(x.is_alive() for x in th), "a rank did not return"
        return out, time.monotonic() - t0

    def clean():
        out, _ = on_ranks()
        for text, words in out:
            assert text is None, text
            same(machine_ref_words, words, "two thread-ranks")
    try:
        clean()                                  # kernels compiled
        live0, c0 = [_live(b) for b in bes], bes[1].get_option("debug.alloc_count")
        clean()
        n = bes[1].get_option("debug.alloc_count") - c0
        assert n >= 8
        longest = 0.0
        for k in range(1, n + 1):
            bes[1].set_option("debug.fail_alloc", k)
            out, took = on_ranks()
            longest = max(longest, took)
            assert bes[1].get_option("debug.fail_alloc") == 0, k
            assert out[1][0] is not None and _is_injection(out[1][0], k), (k, out[1])
            if out[0][0] is None:                # rank 1 was refused behind its last collective: rank 0 had everything it needed
                same(machine_ref_words, out[0][1], ("rank 0", k))
            assert took < SHARDED_TIMEOUT_MS / 2000, (k, took, "a rank waited for the timeout")
            assert group.broken(), (k, "the refusal on rank 1 did not reach the transport")
            assert [_live(b, want) for b, want in zip(bes, live0)] == live0, k
            group.reset()
            assert not group.broken()
        print(f"two thread-ranks: {n} allocator requests on rank 1, longest call {longest * 1000:.0f} ms of a timeout of {SHARDED_TIMEOUT_MS} ms")
        clean()
        assert [_live(b) for b in bes] == live0
    finally:
        for r in range(world):
            bes[r].free_local_comm(comms[r]); bes[r].close()
        group.close()


# ---------------------------------------------------------------------------------------------------------------- 6. plumbing

def test_option_plumbing(nz, monkeypatch):
    b = nz.HipBackend(0)
    try:
        assert [b.get_option(n) for n in ("mem.limit_bytes", "mem.cache_bytes", "mem.cached_bytes", "debug.fail_alloc", "debug.alloc_count")] == [0, 192 << 30, 0, 0, 0]
        for name, bad in (("mem.limit_bytes", -1), ("mem.limit_bytes", (1 << 62) + 1), ("mem.cache_bytes", -1), ("mem.cache_bytes", (1 << 62) + 1), ("debug.fail_alloc", -1),
                          ("debug.fail_alloc", (1 << 30) + 1), ("debug.alloc_count", 0), ("debug.alloc_count", 5), ("mem.cached_bytes", 0), ("mem.no_such_option", 1)):
            before = b.get_option(name) if name != "mem.no_such_option" else None
            with pytest.raises(nz.NexusHipError) as e:
                b.set_option(name, bad)
            assert f"error {NX_ERR_ARG}:" in str(e.value) and name in str(e.value)
            assert name == "mem.no_such_option" or b.get_option(name) == before
        with pytest.raises(nz.NexusHipError):
            b.get_option("mem.no_such_option")
        b.set_option("mem.limit_bytes", 1 << 40); b.set_option("mem.cache_bytes", 1 << 62)
        assert b.get_option("mem.limit_bytes") == 1 << 40 and b.get_option("mem.cache_bytes") == 1 << 62
        b.set_option("mem.limit_bytes", 0)
        # the counter counts requests, refused ones too; the injection counts from where it is armed
        p, q = C.c_void_p(), C.c_void_p()
        b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(3), C.byref(p)))
        assert b.get_option("debug.alloc_count") == 1
        b.set_option("debug.fail_alloc", 2)
        assert b.get_option("debug.fail_alloc") == 2
        b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(3), C.byref(q)))
        assert b.get_option("debug.fail_alloc") == 2
        b._chk(b.L.nx_free(b.ctx, q))
        assert b.L.nx_alloc(b.ctx, C.c_size_t(65), C.byref(q)) == NX_ERR_OOM and not q.value
        assert b.L.nx_last_error(b.ctx).decode() == "debug.fail_alloc: request 2 (512 bytes) refused"
        assert b.get_option("debug.fail_alloc") == 0 and b.get_option("debug.alloc_count") == 3
        b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(65), C.byref(q)))      # refused once
        b.set_option("debug.fail_alloc", 5); b.set_option("debug.fail_alloc", 0)      # disarmed
        b._chk(b.L.nx_free(b.ctx, p)); b._chk(b.L.nx_free(b.ctx, q))
        assert b.memory()[0] == 0 and b.get_option("mem.cached_bytes") == 256 + 256 + 512
    finally:
        b.close()
    monkeypatch.setenv("NX_MEM_LIMIT_BYTES", str(40 << 30))
    monkeypatch.setenv("NX_MEM_CACHE_BYTES", "0")
    b = nz.HipBackend(0)
    try:
        assert b.get_option("mem.limit_bytes") == 40 << 30 and b.get_option("mem.cache_bytes") == 0 and b.get_option("debug.fail_alloc") == 0
        p = C.c_void_p()
        b._chk(b.L.nx_alloc(b.ctx, C.c_size_t(64), C.byref(p)))
        b._chk(b.L.nx_free(b.ctx, p))
        assert b.get_option("mem.cached_bytes") == 0
    finally:
        b.close()
