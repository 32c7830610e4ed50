"""nx_trace_keccak_round on the device against the byte-wise model of tests/keccak_round_model.py: every word of d_main, d_pre and
d_states_out at every shape of the model's list, two chained calls against hashlib, NULL outputs, determinism, memory — and a keccak
statement with the reference's constraints and relation entries (tests/keccak_air.py) filled on the device, checked, balanced, proved
and verified."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import keccak_round_model as M
from keccak_air import (COMPONENTS, COMP_LOG, INTER_AT, KEY_BITS, LOG_A, LOG_B, LOG_BIT, MAIN_AT, N_INST, N_INT, N_MAIN, N_PRE, PRE_AT, TREE_LOGS,
                        host_statement, statement_programs, total)

pytestmark = pytest.mark.gpu
P = M.P
GUARD = 0xDEADBEEF


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


def _states_on_device(be, nz, states):
    """(n, 25) uint64 -> device words (a slab of at least one column); the lanes are little-endian pairs of words"""
    words = np.ascontiguousarray(states, "<u8").view(np.uint32).reshape(-1)
    log = max(1, int(max(1, len(words)) - 1).bit_length())
    buf = np.full(1 << log, GUARD, np.uint32)
    buf[:len(words)] = words
    return nz.DeviceColumns(be, 1, log).upload(buf[None, :])


def _lanes(dev, n_instances):
    return dev.to_cpu().reshape(-1)[:50 * n_instances].view("<u8").reshape(n_instances, 25)


def run(be, nz, states, first_round, log_rounds, log_size, want_pre=True, want_out=True):
    """the call into guard-filled columns -> (main, pre or None, out or None, the word behind the output lanes)"""
    n_inst = len(states)
    d_in = _states_on_device(be, nz, states)
    main = nz.DeviceColumns(be, M.MAIN_COLS, log_size).upload(np.full((M.MAIN_COLS, 1 << log_size), GUARD, np.uint32))
    pre = nz.DeviceColumns(be, M.PRE_COLS, log_size).upload(np.full((M.PRE_COLS, 1 << log_size), GUARD, np.uint32)) if want_pre else None
    d_out = _states_on_device(be, nz, np.full((max(1, n_inst), 25), GUARD | (GUARD << 32), np.uint64)) if want_out else None
    be.trace_keccak_round(d_in.ptr.value if n_inst else None, n_inst, first_round, log_rounds, log_size, list(main.col_ptrs()),
                          list(pre.col_ptrs()) if pre else None, d_out.ptr.value if d_out else None)
    assert np.array_equal(_lanes(d_in, n_inst), states)               # the inputs are left alone
    return main.to_cpu(), pre.to_cpu() if pre else None, _lanes(d_out, n_inst) if d_out else None, d_out.to_cpu().reshape(-1) if d_out else None


def _same(got, want, what):
    for k in np.flatnonzero((got != want).any(axis=1))[:1]:
        raise AssertionError("%s column %d differs at positions %s" % (what, k, np.flatnonzero(got[k] != want[k])[:8]))


@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_every_word_equals_the_models(be, nz, shape):
    n_inst, first, log_rounds, log_size = shape
    states = M.test_states(n_inst, seed=log_size)
    want = M.fill(states, first, log_rounds, log_size)
    main, pre, out, raw = run(be, nz, states, first, log_rounds, log_size)
    _same(main, want["main"], "main")
    _same(pre, want["pre"], "preprocessed")
    assert np.array_equal(out, want["out"])
    assert (raw[50 * n_inst:] == GUARD).all()                         # nothing behind the last instance's lanes


def test_two_chained_calls_are_keccak_f_of_a_sha3_block(be, nz):
    msgs = [b"", b"abc", bytes(range(135))]
    states = np.stack([M.sha3_256_block(m) for m in msgs])
    _, _, mid, _ = run(be, nz, states, 0, 4, 6)
    _, _, out, _ = run(be, nz, mid, 16, 3, 5)
    for m, s in zip(msgs, out):
        assert M.digest(s) == hashlib.sha3_256(m).digest()


def test_pre_and_states_out_may_be_null(be, nz):
    states = M.test_states(3, seed=1)
    want = M.fill(states, 0, 4, 6)
    main, pre, out, _ = run(be, nz, states, 0, 4, 6, want_pre=False, want_out=False)
    _same(main, want["main"], "main")
    assert pre is None and out is None
    main, pre, out, _ = run(be, nz, states, 0, 4, 6, want_pre=True, want_out=False)
    _same(main, want["main"], "main")
    _same(pre, want["pre"], "preprocessed")


def test_same_words_on_two_runs_and_no_device_memory_is_taken(be, nz):
    states = M.test_states(17, seed=2)
    d_in = _states_on_device(be, nz, states)
    main = nz.DeviceColumns(be, M.MAIN_COLS, 9)
    pre = nz.DeviceColumns(be, M.PRE_COLS, 9)
    d_out = _states_on_device(be, nz, np.zeros((17, 25), np.uint64))
    be.sync()
    runs = []
    for _ in range(2):
        main.upload(np.full((M.MAIN_COLS, 512), GUARD, np.uint32))
        before = be.memory(reset_peak=True)
        be.trace_keccak_round(d_in.ptr.value, 17, 0, 4, 9, list(main.col_ptrs()), list(pre.col_ptrs()), d_out.ptr.value)
        be.sync()
        live, peak = be.memory()
        assert (live, peak) == (before[0], before[0])                 # nothing allocated, not even for the length of the call
        runs.append((main.to_cpu(), pre.to_cpu(), _lanes(d_out, 17).copy()))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    assert not (runs[0][0] == GUARD).any()


# ------------------------------------------------------------------------------- a keccak statement through the session ----------
# (layout, programs and the model's columns: tests/keccak_air.py)
def _upload(be, ptr, host):
    host = np.ascontiguousarray(host, np.uint32)
    be._chk(be.L.nx_upload(be.ctx, C.c_void_p(ptr), host.ctypes.data_as(C.c_void_p), C.c_size_t(len(host))))


def _download(be, nz, ptr, log):
    return nz.DeviceColumns.view(be, ptr, 1, log).to_cpu().reshape(-1)


def _keep(be, nz, ptrs, log):
    """the columns cloned into one slab (a commit turns its columns into coefficients) -> their addresses in the slab"""
    slab = nz.DeviceColumns(be, len(ptrs), log)
    for k, p in enumerate(ptrs):
        be._chk(be.L.nx_copy(be.ctx, C.c_void_p(slab.ptr.value + k * (4 << log)), C.c_void_p(p), C.c_size_t(1 << log)))
    return slab, [slab.ptr.value + k * (4 << log) for k in range(len(ptrs))]


def _keccak_session(be, nz, states, tamper=False):
    """The statement filled on the device.  -> (claimed sums by component, None) when tamper, else (claimed, everything the test needs)"""
    import nexus_zkvm_amd.air_program as ap
    import keccak_air as K
    cfg = nz.default_config(pow_bits=2)
    host_pre, host_main, final = host_statement(states)
    s = be.prover_session(cfg, LOG_BIT)
    s.mix_u64(5)
    # tree 0: the round components' preprocessed columns come from the device call (no instances, the main columns into a scratch slab)
    pre = s.tree_begin(TREE_LOGS[0])
    for name, first, log_rounds in (("round_a", 0, 4), ("round_b", 16, 3)):
        scratch = nz.DeviceColumns(be, M.MAIN_COLS, COMP_LOG[name])
        be.trace_keccak_round(None, 0, first, log_rounds, COMP_LOG[name], list(scratch.col_ptrs()), pre[PRE_AT[name]:PRE_AT[name] + 9], None)
    for d, col in zip(pre[18:], host_pre[18:]):
        _upload(be, d, col)
    keep_pre = {name: _keep(be, nz, pre[PRE_AT[name]:PRE_AT[name] + N_PRE[name]], COMP_LOG[name]) for name in PRE_AT}
    roots = [s.tree_commit()]
    # tree 1: both round traces straight into the tree's columns, the second component fed the first's output states
    main = s.tree_begin(TREE_LOGS[1])
    d_in, d_mid, d_fin = (_states_on_device(be, nz, x) for x in (states, np.zeros((N_INST, 25), np.uint64), np.zeros((N_INST, 25), np.uint64)))
    be.trace_keccak_round(d_in.ptr.value, N_INST, 0, 4, LOG_A, main[:1705], None, d_mid.ptr.value)
    be.trace_keccak_round(d_mid.ptr.value, N_INST, 16, 3, LOG_B, main[1705:3410], None, d_fin.ptr.value)
    assert np.array_equal(_lanes(d_fin, N_INST), final)
    if tamper:                                                           # one byte of the first theta xor of natural row 0
        col = _download(be, nz, main[200], LOG_A)
        col[0] ^= 1
        _upload(be, main[200], col)
    # multiplicities from the device-filled columns, weights NULL: every row looks up, padding included; a rotate use has its shift
    # amount as a scratch constant column
    shift_cols = nz.DeviceColumns(be, 8, LOG_A).upload(np.repeat(np.arange(8, dtype=np.uint32)[:, None], 1 << LOG_A, axis=1))
    lookups = K.round_program(ap, {name: ((1, 0, 0, 0), (2, 0, 0, 0)) for name, _ in K.RELATIONS}, (0, 0, 0, 0))[1]
    uses = {"xor": [], "not_and": [], "rotate": []}
    for name in ("round_a", "round_b"):
        col = lambda k: main[MAIN_AT[name] + k] if k < M.MAIN_COLS else keep_pre[name][1][k - M.MAIN_COLS]
        for t in ("xor", "not_and"):
            uses[t] += [([col(a), col(b)], None, COMP_LOG[name]) for a, b, _ in lookups[t]]
        uses["rotate"] += [([col(a), shift_cols.ptr.value + bits * (4 << LOG_A)], None, COMP_LOG[name]) for a, bits, _, _ in lookups["rotate"]]
    for t in ("xor", "not_and", "rotate"):
        assert be.logup_multiplicities(uses[t], keep_pre[t][1][:2], COMP_LOG[t], KEY_BITS[t], main[MAIN_AT[t]]) == (0, 0, 0)
    for d, col in zip(main[3413:], host_main[3413:]):
        _upload(be, d, col)
    if not tamper:
        for k in list(range(0, 3410, 97)) + [1704, 3409, 3410, 3411, 3412]:
            assert np.array_equal(_download(be, nz, main[k], TREE_LOGS[1][k]), host_main[k]), "main column %d" % k
    keep_main = {name: _keep(be, nz, main[MAIN_AT[name]:MAIN_AT[name] + N_MAIN[name]], COMP_LOG[name]) for name in COMPONENTS}
    roots.append(s.tree_commit())
    drawn = s.draw_felts(8)
    elems = {name: (drawn[2 * k], drawn[2 * k + 1]) for k, (name, _) in enumerate(K.RELATIONS)}
    # tree 2: the interaction trace of every component from its recorded relation entries
    fracs = statement_programs(ap, elems, {name: (0, 0, 0, 0) for name in COMPONENTS})
    inter = s.tree_begin(TREE_LOGS[2])
    claimed, shifts = {}, {}
    for name in COMPONENTS:
        log, out = COMP_LOG[name], inter[INTER_AT[name]:INTER_AT[name] + N_INT[name]]
        cols = keep_main[name][1] + (keep_pre[name][1] if N_PRE[name] else [])
        if name in ("xor", "not_and", "rotate"):
            cols = keep_pre[name][1] + keep_main[name][1]                # a table program reads its tuple first
        frac = fracs[name].build_logup()
        assert 4 * frac.n_logup_cols == len(out)
        be.logup_program(frac, cols + [None] * len(out), log, out_ptrs=out)
        claimed[name] = be.logup_finalize_last(out[-4:], log_size=log)
        n_inv = pow((1 << log) % P, P - 2, P)
        shifts[name] = [(int(x) * n_inv) % P for x in claimed[name]]
    if tamper:
        s.close()
        return claimed, None
    s.mix_felts(np.array([claimed[name] for name in COMPONENTS], np.uint32))
    roots.append(s.tree_commit())
    progs = statement_programs(ap, elems, shifts)
    built = {name: progs[name].build() for name in COMPONENTS}
    assert np.array_equal(built["round_a"].instrs, built["round_b"].instrs)   # one program for both round components: one compile
    comps = []
    for name in COMPONENTS:
        pre_c, main_c = [(0, PRE_AT[name] + k) for k in range(N_PRE[name])], [(1, MAIN_AT[name] + k) for k in range(N_MAIN[name])]
        order = pre_c + main_c if name in ("xor", "not_and", "rotate") else main_c + pre_c
        comps.append(ap.Component(COMP_LOG[name], built[name], order + [(2, INTER_AT[name] + k) for k in range(N_INT[name])]))
    return claimed, (s, cfg, comps, roots, drawn, host_pre, host_main)


@pytest.fixture(scope="module")
def statement(be, nz):
    states = M.test_states(N_INST, seed=7)
    states[0] = M.sha3_256_block(b"keccak")
    return states, _keccak_session(be, nz, states)


def test_a_keccak_statement_filled_on_the_device_is_proved_and_verified(be, nz, statement):
    states, (claimed, (s, cfg, comps, roots, drawn, host_pre, host_main)) = statement
    assert total(claimed) == [0, 0, 0, 0]                              # the reference verifier's zero-sum rule (machine.rs:343)
    assert all(np.asarray(claimed[name]).any() for name in COMPONENTS)
    report = s.check(comps)
    assert report.ok, report
    words = s.prove(comps)
    v = nz.VerifierSession(cfg)
    v.mix_u64(5)
    v.commit(roots[0], TREE_LOGS[0])
    v.commit(roots[1], TREE_LOGS[1])
    assert np.array_equal(v.draw_felts(8), drawn)
    v.mix_felts(np.array([claimed[name] for name in COMPONENTS], np.uint32))
    v.commit(roots[2], TREE_LOGS[2])
    assert v.verify(comps, words) is None
    assert np.array_equal(v.digest(), s.digest())
    s.close()
    # the same preprocessed and main trees from a session fed the model's columns by the host: byte-equal roots
    h = be.prover_session(cfg, LOG_BIT)
    h.mix_u64(5)
    assert np.array_equal(h.commit(host_pre), roots[0])
    assert np.array_equal(h.commit(host_main), roots[1])
    h.close()
    # the control: one device-filled word changed before the commit and the sums no longer cancel
    off, _ = _keccak_session(be, nz, states, tamper=True)
    assert total(off) != [0, 0, 0, 0]
