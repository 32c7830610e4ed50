"""nx_trace_keccak_memory_check on the device against the model of tests/keccak_memcheck_model.py: every word of d_main, d_pre and
d_states_out at every shape of the model's list, NULL outputs, the permuted states against two chained nx_trace_keccak_round calls,
determinism, memory — and the CLOSED keccak statement (tests/keccak_memcheck_air.py): the reference's six components with the
reference's constraints, every main column of the keccak extension filled on the device, checked, balanced, proved and verified."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import keccak_memcheck_model as MM
import keccak_round_model as M
from keccak_memcheck_air import (COMPONENTS, COMP_LOG, INTER_AT, KEY_BITS, LOG_A, LOG_B, LOG_BIT, LOG_MC, MAIN_AT, N_INST, N_INT, N_MAIN, N_PRE, PRE_AT, RELATIONS,
                                 TREE_LOGS, host_statement, statement_inputs, statement_programs, total)
from test_gpu_keccak_round import GUARD, _download, _keep, _lanes, _same, _states_on_device, _upload
from test_gpu_keccak_round import run as run_round

pytestmark = pytest.mark.gpu
P = M.P
SHAPE_IDS = [MM.shape_id(s) for s in MM.SHAPES]


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


def _words_on_device(be, nz, words):
    """uint32 words -> a device slab of at least one column (256-byte aligned, so 16-byte aligned), guard words behind them"""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1)
    log = max(1, int(max(1, len(words)) - 1).bit_length())
    buf = np.full(1 << log, GUARD, np.uint32)
    buf[:len(words)] = words
    return nz.DeviceColumns(be, 1, log).upload(buf[None, :])


def run(be, nz, states, addresses, timestamps, log_size, want_pre=True, want_out=True):
    """the call into guard-filled columns -> (main, pre or None, out or None, the words of the output buffer)"""
    n_inst = len(states)
    d_in, d_addr, d_ts = _states_on_device(be, nz, states), _words_on_device(be, nz, addresses), _words_on_device(be, nz, timestamps)
    assert d_ts.ptr.value % 16 == 0
    main = nz.DeviceColumns(be, MM.MAIN_COLS, log_size).upload(np.full((MM.MAIN_COLS, 1 << log_size), GUARD, np.uint32))
    pre = nz.DeviceColumns(be, MM.PRE_COLS, log_size).upload(np.full((MM.PRE_COLS, 1 << log_size), GUARD, np.uint32)) if want_pre else None
    d_out = _states_on_device(be, nz, np.full((max(1, n_inst), 25), GUARD | (GUARD << 32), np.uint64)) if want_out else None
    dev = lambda d: d.ptr.value if n_inst else None
    be.trace_keccak_memory_check(dev(d_in), dev(d_addr), dev(d_ts), n_inst, log_size, list(main.col_ptrs()), list(pre.col_ptrs()) if pre else None,
                                 d_out.ptr.value if d_out else None)
    assert np.array_equal(_lanes(d_in, n_inst), states)               # the inputs are left alone
    assert np.array_equal(d_addr.to_cpu().reshape(-1)[:n_inst], addresses) and np.array_equal(d_ts.to_cpu().reshape(-1)[:200 * n_inst], np.asarray(timestamps).reshape(-1))
    return main.to_cpu(), pre.to_cpu() if pre else None, _lanes(d_out, n_inst) if d_out else None, d_out.to_cpu().reshape(-1) if d_out else None


@pytest.mark.parametrize("k", range(len(MM.SHAPES)), ids=SHAPE_IDS)
def test_every_word_equals_the_models(be, nz, k):
    log_size, n_inst = MM.SHAPES[k][:2]
    want = MM.want(k)
    main, pre, out, raw = run(be, nz, *MM.inputs(k), log_size)
    _same(main, want["main"], "main")
    _same(pre, want["pre"], "preprocessed")
    assert np.array_equal(out, want["out"])
    assert (raw[50 * n_inst:] == GUARD).all()                         # nothing behind the last instance's lanes


def test_pre_and_states_out_may_be_null(be, nz):
    want = MM.want(3)
    main, pre, out, _ = run(be, nz, *MM.inputs(3), 2, want_pre=False, want_out=False)
    _same(main, want["main"], "main")
    assert pre is None and out is None
    main, pre, out, _ = run(be, nz, *MM.inputs(3), 2, want_pre=True, want_out=False)
    _same(main, want["main"], "main")
    _same(pre, want["pre"], "preprocessed")
    main, pre, out, _ = run(be, nz, *MM.inputs(3), 2, want_pre=False, want_out=True)
    _same(main, want["main"], "main")
    assert np.array_equal(out, want["out"])


def test_states_out_is_that_of_two_chained_round_calls(be, nz):
    states, addresses, ts = MM.inputs(5)
    _, _, mid, _ = run_round(be, nz, states, 0, 4, 8)                 # 16 rounds, then 8
    _, _, fin, _ = run_round(be, nz, mid, 16, 3, 7)
    _, _, out, _ = run(be, nz, states, addresses, ts, 4)
    assert np.array_equal(out, fin)


def test_same_words_on_two_runs_and_no_device_memory_is_taken(be, nz):
    states, addresses, ts = MM.inputs(6)
    d_in, d_addr, d_ts = _states_on_device(be, nz, states), _words_on_device(be, nz, addresses), _words_on_device(be, nz, ts)
    main = nz.DeviceColumns(be, MM.MAIN_COLS, 9)
    pre = nz.DeviceColumns(be, MM.PRE_COLS, 9)
    d_out = _states_on_device(be, nz, np.zeros((300, 25), np.uint64))
    be.sync()
    runs = []
    for _ in range(2):
        main.upload(np.full((MM.MAIN_COLS, 512), GUARD, np.uint32))
        before = be.memory(reset_peak=True)
        be.trace_keccak_memory_check(d_in.ptr.value, d_addr.ptr.value, d_ts.ptr.value, 300, 9, list(main.col_ptrs()), list(pre.col_ptrs()), d_out.ptr.value)
        be.sync()
        live, peak = be.memory()
        assert (live, peak) == (before[0], before[0])                 # nothing allocated, not even for the length of the call
        runs.append((main.to_cpu(), pre.to_cpu(), _lanes(d_out, 300).copy()))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    assert not (runs[0][0] == GUARD).any()


# ------------------------------------------------------------------------------- the closed statement through the session ----------
# (layout, programs and the models' columns: tests/keccak_memcheck_air.py)
TAMPERED_BYTE, TAMPERED_ROW = 7, 1
TS_CONSTRAINT = 1 + 200 + 2 * TAMPERED_BYTE        # is_padding, the 200 address constraints, then two per byte: the low-limb one of byte 7


def _session(be, nz, inputs, tamper=None):
    """The closed statement filled on the device.  tamper: None; "out": one out_state byte of mem_check changed before the commit ->
    (claimed sums, None); "ts": one next-timestamp limb changed -> the committed session goes as far as the components.
    -> (claimed sums by component, (session, config, components, roots, drawn, host_pre, host_main) or None)"""
    import nexus_zkvm_amd.air_program as ap
    import keccak_air as K
    states, addresses, timestamps = inputs
    cfg = nz.default_config(pow_bits=2)
    host_pre, host_main, final = host_statement(states, addresses, timestamps)
    s = be.prover_session(cfg, LOG_BIT)
    s.mix_u64(5)
    # tree 0: the preprocessed columns of the three device-filled components come from the device calls (no instances, the main columns
    # into a scratch slab)
    pre = s.tree_begin(TREE_LOGS[0])
    for name, first, log_rounds in (("round_a", 0, 4), ("round_b", 16, 3)):
        scratch = nz.DeviceColumns(be, M.MAIN_COLS, COMP_LOG[name])
        be.trace_keccak_round(None, 0, first, log_rounds, COMP_LOG[name], list(scratch.col_ptrs()), pre[PRE_AT[name]:PRE_AT[name] + 9], None)
    scratch = nz.DeviceColumns(be, MM.MAIN_COLS, LOG_MC)
    be.trace_keccak_memory_check(None, None, None, 0, LOG_MC, list(scratch.col_ptrs()), pre[PRE_AT["mem_check"]:PRE_AT["mem_check"] + 1], None)
    for d, col in zip(pre[18:28], host_pre[18:28]):
        _upload(be, d, col)
    keep_pre = {name: _keep(be, nz, pre[PRE_AT[name]:PRE_AT[name] + N_PRE[name]], COMP_LOG[name]) for name in PRE_AT}
    roots = [s.tree_commit()]
    # tree 1: both round traces and the memory-check trace straight into the tree's columns, from ONE buffer of input states
    main = s.tree_begin(TREE_LOGS[1])
    zeros = np.zeros((N_INST, 25), np.uint64)
    d_in, d_mid, d_fin, d_mc = (_states_on_device(be, nz, x) for x in (states, zeros, zeros, zeros))
    d_addr, d_ts = _words_on_device(be, nz, addresses), _words_on_device(be, nz, timestamps)
    at = MAIN_AT["mem_check"]
    be.trace_keccak_round(d_in.ptr.value, N_INST, 0, 4, LOG_A, main[:1705], None, d_mid.ptr.value)
    be.trace_keccak_round(d_mid.ptr.value, N_INST, 16, 3, LOG_B, main[1705:3410], None, d_fin.ptr.value)
    be.trace_keccak_memory_check(d_in.ptr.value, d_addr.ptr.value, d_ts.ptr.value, N_INST, LOG_MC, main[at:at + MM.MAIN_COLS], None, d_mc.ptr.value)
    assert np.array_equal(_lanes(d_fin, N_INST), final) and np.array_equal(_lanes(d_mc, N_INST), final)
    if tamper:
        k = at + (MM.OUT + 17 if tamper == "out" else MM.NEXT_TS + 2 * TAMPERED_BYTE)
        col = _download(be, nz, main[k], LOG_MC)
        col[int(M.pos_of_coset_row(TAMPERED_ROW, LOG_MC))] ^= 1
        _upload(be, main[k], col)
    # multiplicities from the device-filled columns, as tests/test_gpu_keccak_round.py counts them
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
    for d, col in zip(main[MAIN_AT["mem_side"]:], host_main[MAIN_AT["mem_side"]:]):      # the stand-in for the load/store chip: from the host
        _upload(be, d, col)
    if not tamper:
        for k in list(range(0, at + MM.MAIN_COLS, 97)) + [1704, 3409, 3410, 3411, 3412, at + MM.IS_PADDING]:
            assert np.array_equal(_download(be, nz, main[k], TREE_LOGS[1][k]), host_main[k]), "main column %d" % k
    keep_main = {name: _keep(be, nz, main[MAIN_AT[name]:MAIN_AT[name] + N_MAIN[name]], COMP_LOG[name]) for name in COMPONENTS}
    roots.append(s.tree_commit())
    drawn = s.draw_felts(2 * len(RELATIONS))
    elems = {name: (drawn[2 * k], drawn[2 * k + 1]) for k, (name, _) in enumerate(RELATIONS)}
    # tree 2: the interaction trace of every component from its recorded relation entries
    fracs = statement_programs(ap, elems, {name: (0, 0, 0, 0) for name in COMPONENTS})
    inter = s.tree_begin(TREE_LOGS[2])
    claimed, shifts = {}, {}
    for name in COMPONENTS:
        log, out = COMP_LOG[name], inter[INTER_AT[name]:INTER_AT[name] + N_INT[name]]
        cols = keep_main[name][1] + (keep_pre[name][1] if N_PRE[name] else [])
        if name in KEY_BITS:
            cols = keep_pre[name][1] + keep_main[name][1]                # a table program reads its tuple first
        frac = fracs[name].build_logup()
        assert 4 * frac.n_logup_cols == len(out)
        be.logup_program(frac, cols + [None] * len(out), log, out_ptrs=out)
        claimed[name] = be.logup_finalize_last(out[-4:], log_size=log)
        n_inv = pow((1 << log) % P, P - 2, P)
        shifts[name] = [(int(x) * n_inv) % P for x in claimed[name]]
    if tamper == "out":
        s.close()
        return claimed, None
    s.mix_felts(np.array([claimed[name] for name in COMPONENTS], np.uint32))
    roots.append(s.tree_commit())
    progs = statement_programs(ap, elems, shifts)
    built = {name: progs[name].build() for name in COMPONENTS}
    comps = []
    for name in COMPONENTS:
        pre_c, main_c = [(0, PRE_AT[name] + k) for k in range(N_PRE[name])], [(1, MAIN_AT[name] + k) for k in range(N_MAIN[name])]
        order = pre_c + main_c if name in KEY_BITS else main_c + pre_c
        comps.append(ap.Component(COMP_LOG[name], built[name], order + [(2, INTER_AT[name] + k) for k in range(N_INT[name])]))
    return claimed, (s, cfg, comps, roots, drawn, host_pre, host_main)


@pytest.fixture(scope="module")
def statement(be, nz):
    inputs = statement_inputs()
    return inputs, _session(be, nz, inputs)


def test_the_closed_keccak_statement_filled_on_the_device_is_proved_and_verified(be, nz, statement):
    inputs, (claimed, (s, cfg, comps, roots, drawn, host_pre, host_main)) = statement
    assert total(claimed) == [0, 0, 0, 0]                              # the reference verifier's zero-sum rule (machine.rs:343)
    assert all(np.asarray(claimed[name]).any() for name in COMPONENTS)
    report = s.check(comps)
    assert report.ok, report
    words = s.prove(comps)
    v = nz.VerifierSession(cfg)
    v.mix_u64(5)
    v.commit(roots[0], TREE_LOGS[0])
    v.commit(roots[1], TREE_LOGS[1])
    assert np.array_equal(v.draw_felts(2 * len(RELATIONS)), drawn)
    v.mix_felts(np.array([claimed[name] for name in COMPONENTS], np.uint32))
    v.commit(roots[2], TREE_LOGS[2])
    assert v.verify(comps, words) is None
    assert np.array_equal(v.digest(), s.digest())
    s.close()
    # the same preprocessed and main trees from a session fed the models' columns by the host: byte-equal roots
    h = be.prover_session(cfg, LOG_BIT)
    h.mix_u64(5)
    assert np.array_equal(h.commit(host_pre), roots[0])
    assert np.array_equal(h.commit(host_main), roots[1])
    h.close()


def test_one_changed_next_timestamp_limb_is_named_by_the_check(be, nz, statement):
    inputs, _ = statement
    _, (s, cfg, comps, roots, drawn, host_pre, host_main) = _session(be, nz, inputs, tamper="ts")
    report = s.check(comps)
    s.close()
    assert not report.ok and report.n_failed == 1, report
    f = report.failures[0]
    assert (f.component, f.constraint, f.first_row, f.n_rows) == (COMPONENTS.index("mem_check"), TS_CONSTRAINT, TAMPERED_ROW, 1), report
    assert report.message.endswith("component %d constraint %d: not zero on 1 of 4 rows, first at row %d" % (COMPONENTS.index("mem_check"), TS_CONSTRAINT, TAMPERED_ROW))


def test_one_changed_out_state_byte_and_the_sums_no_longer_cancel(be, nz, statement):
    inputs, _ = statement
    off, _ = _session(be, nz, inputs, tamper="out")
    assert total(off) != [0, 0, 0, 0]
