"""The narrow host-trace upload on the GPU (-m gpu): byte and half-word limb columns cross PCIe narrow and are widened on the device
(widen_kernel), directly from uint8 / uint16 arrays or packed on host threads from the reference's uint32 layout (NX_COL_U32_AS_*).
Every result is compared with the u32 path or the CPU oracle: numpy widening (+ R3's finalize_column for coset order) for
nx_upload_columns_narrow, the oracle ProverSession's bytes for a real byte-limb AIR committed through the session, nx_prove_machine's bytes
for the machine; a value that does not fit is refused with its column and row, and the same context / session then proves correctly."""
import re
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import oracle_lib as O

pytestmark = pytest.mark.gpu
P = O.P


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    yield b
    b.close()


def _same(ref, words):
    assert len(ref) == len(words), (len(ref), len(words))
    if not np.array_equal(ref, words):
        pytest.fail(f"first differing proof word {int(np.nonzero(ref != words)[0][0])} of {len(ref)}")


# ---------------------------------------------------------------------------------------------------------- 1. nx_upload_columns_narrow
def _mixed_columns(log, rng):
    """one column of every kind: (array handed to the library, as_kind entry, expected u32 values)"""
    n = 1 << log
    u8 = rng.integers(0, 256, n, dtype=np.uint32)
    u16 = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    full = rng.integers(0, P, n, dtype=np.uint32)
    as8 = rng.integers(0, 256, n, dtype=np.uint32)
    as16 = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    u8[0], u16[-1], as8[-1], as16[0] = 255, 65535, 255, 65535
    return [(u8.astype(np.uint8), None, u8), (u16.astype(np.uint16), None, u16), (full, None, full), (as8, np.uint8, as8), (as16, np.uint16, as16)]


@pytest.mark.parametrize("coset_order", [False, True])
def test_upload_mixed_kinds_every_small_size(be, nz, oracle, coset_order):
    rng = np.random.default_rng(3)
    for log in (1, 2, 3, 5, 12, 16):
        cols = [c for _ in range(4) for c in _mixed_columns(log, rng)]      # 20 columns: two 16-column chunks, both staging slots
        got = be.upload_columns_narrow([c for c, _, _ in cols], coset_order=coset_order, as_kind=[a for _, a, _ in cols]).to_cpu()
        for k, (_, _, want) in enumerate(cols):
            want = O.finalize_column(want) if coset_order else want
            assert np.array_equal(got[k], want), (log, k, coset_order)


def test_upload_odd_offset_views_and_owner_pinned_columns(be, nz, oracle):
    rng = np.random.default_rng(4)
    log = 13
    n = 1 << log
    raw = rng.integers(0, 256, 2 * n + 8, dtype=np.uint8)
    v8 = raw[1:1 + n]                                              # a view at an odd byte offset of a larger buffer
    v16 = np.frombuffer(raw.tobytes(), dtype=np.uint16, offset=3, count=n)   # an unaligned uint16 view
    pinned8 = rng.integers(0, 256, n, dtype=np.uint8)
    pinned16 = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    be.host_pin(pinned8)
    be.host_pin(pinned16)
    try:
        for coset_order in (False, True):
            cols = [v8, v16, pinned8, pinned16]
            got = be.upload_columns_narrow(cols, coset_order=coset_order).to_cpu()
            for k, c in enumerate(cols):
                want = c.astype(np.uint32)
                assert np.array_equal(got[k], O.finalize_column(want) if coset_order else want), (k, coset_order)
    finally:
        be.host_unpin(pinned8)
        be.host_unpin(pinned16)


def test_upload_refuses_values_that_do_not_fit_and_the_context_stays_usable(be, nz):
    rng = np.random.default_rng(5)
    log = 17
    n = 1 << log
    cols = [rng.integers(0, 256, n, dtype=np.uint32) for _ in range(20)]
    before = [c.copy() for c in cols]
    cols[18][7] = 256                    # the third chunk's ...
    cols[17][n - 1] = 1 << 20            # ... lowest column wins, then the lowest row
    cols[17][n - 5] = 300
    for threads in (1, 16):
        be.set_option("host.pack_threads", threads)
        with pytest.raises(nz.NexusHipError) as e:
            be.upload_columns_narrow(cols, coset_order=False, as_kind=np.uint8)
        msg = str(e.value)
        assert "column 17, row %d" % (n - 5) in msg and "300" in msg and "NX_COL_U32_AS_U8" in msg, msg
    be.set_option("host.pack_threads", 16)
    assert all(np.array_equal(a, b) for a, b in zip(cols[:17] + cols[19:], before[:17] + before[19:]))   # the caller's arrays are read only
    cols[17][n - 1], cols[17][n - 5], cols[18][7] = 1, 2, 3
    got = be.upload_columns_narrow(cols, coset_order=True, as_kind=np.uint8).to_cpu()
    for k in (0, 17, 18):
        assert np.array_equal(got[k], O.finalize_column(cols[k])), k


# ---------------------------------------------------------------------------------- 2. session, a byte-limb AIR (b0..b3, h0, h1, w)
GROUPS = 5          # 7-column groups per component: 35 columns, across the 16-column chunk boundary


def _limb_component(ap, log, main0):
    """w = sum 2^(8k) b_k and w = h0 + 2^16 h1, GROUPS times"""
    pb = ap.ProgramBuilder()
    for g in range(GROUPS):
        b = [pb.next_trace_mask(7 * g + k)[0] for k in range(4)]
        h = [pb.next_trace_mask(7 * g + 4 + k)[0] for k in range(2)]
        (w,) = pb.next_trace_mask(7 * g + 6)
        pb.add_constraint(w - (b[0] + b[1] * (1 << 8) + b[2] * (1 << 16) + b[3] * (1 << 24)))
        pb.add_constraint(w - (h[0] + h[1] * (1 << 16)))
    return ap.Component(log, pb.build(), [(1, main0 + k) for k in range(7 * GROUPS)])


def _limb_trace(log, seed):
    """natural-order columns of one component: u32 arrays, and the narrow form (uint8 limbs, uint16 halves, uint32 w)"""
    rng = np.random.default_rng(seed)
    n = 1 << log
    wide, narrow = [], []
    for _ in range(GROUPS):
        w = rng.integers(0, 1 << 31, n, dtype=np.uint64)
        w[w == P] = 0                                            # top byte below 128, and a canonical field element
        w = w.astype(np.uint32)
        limbs = [(w >> (8 * k)) & 0xff for k in range(4)] + [w & 0xffff, w >> 16]
        wide += [x.astype(np.uint32) for x in limbs] + [w]
        narrow += [x.astype(np.uint8) for x in limbs[:4]] + [x.astype(np.uint16) for x in limbs[4:]] + [w]
    return wide, narrow


LOGS = (8, 6)
AS_KIND = ([np.uint8] * 4 + [np.uint16] * 2 + [None]) * GROUPS * len(LOGS)


def _statement(seed=21):
    wide, narrow = [], []
    for i, log in enumerate(LOGS):
        w, n = _limb_trace(log, seed + i)
        wide += w; narrow += n
    return wide, narrow


def _drive(session, ap, commit_main):
    session.mix_u64(max(LOGS))
    session.commit([])
    commit_main()
    comps, main0 = [], 0
    for log in LOGS:
        comps.append(_limb_component(ap, log, main0)); main0 += 7 * GROUPS
    return session.prove(comps)


def _reference(nz, ap, wide):
    ocfg = O.default_cfg(pow_bits=4)
    o = O.ProverSession(ocfg, max(LOGS))
    return _drive(o, ap, lambda: o.commit([O.finalize_column(c) for c in wide]))


def test_session_byte_limb_air_from_narrow_columns_equals_the_oracle(be, nz, oracle):
    import nexus_zkvm_amd.air_program as ap
    wide, narrow = _statement()
    ref = _reference(nz, ap, wide)
    cfg = nz.default_config(pow_bits=4)
    fin = [O.finalize_column(c) for c in wide]
    keep = (0, 40)
    variants = {
        "commit_host u32": lambda s: s.commit_host(fin, keep=keep),
        "narrow arrays, circle order": lambda s: s.commit_host_narrow([O.finalize_column(c).astype(c.dtype) for c in narrow], keep=keep),
        "narrow arrays, coset order": lambda s: s.commit_host_narrow(narrow, coset_order=True, keep=keep),
        "u32 as_kind, circle order": lambda s: s.commit_host_narrow(fin, keep=keep, as_kind=AS_KIND),
        "u32 as_kind, coset order": lambda s: s.commit_host_narrow(wide, coset_order=True, keep=keep, as_kind=AS_KIND),
    }
    for name, commit in variants.items():
        s = be.prover_session(cfg, max(LOGS))
        kept = {}
        try:
            _same(ref, _drive(s, ap, lambda: kept.update(commit(s)[1])))
            for k in keep:
                assert np.array_equal(kept[k].to_cpu()[0], fin[k]), (name, k)
        finally:
            s.close()


def test_session_refused_commit_then_corrected_commit_equals_the_oracle(be, nz, oracle):
    import nexus_zkvm_amd.air_program as ap
    wide, narrow = _statement(seed=23)
    ref = _reference(nz, ap, wide)
    s = be.prover_session(nz.default_config(pow_bits=4), max(LOGS))
    try:
        def commit_main():
            bad = list(AS_KIND)
            bad[6] = np.uint8                                        # w declared a byte: refused, nothing mixed
            with pytest.raises(nz.NexusHipError) as e:
                s.commit_host_narrow(wide, coset_order=True, as_kind=bad)
            assert re.search(r"column 6, row \d+", str(e.value)), str(e.value)
            s.commit_host_narrow(wide, coset_order=True, as_kind=AS_KIND)     # tree_begin of the same tree again, corrected
        _same(ref, _drive(s, ap, commit_main))
    finally:
        s.close()


def test_sharded_session_commit_host_narrow_equals_one_gpu(be, nz, oracle):
    import nexus_zkvm_amd.air_program as ap
    wide, narrow = _statement(seed=25)
    cfg = nz.default_config(pow_bits=4)
    s = be.prover_session(cfg, max(LOGS))
    try:
        one = _drive(s, ap, lambda: s.commit_host_narrow(narrow, coset_order=True))
    finally:
        s.close()
    world = 2
    group = nz.LocalGroup(world)
    results, errors = [None] * world, []

    def run(rank):
        b = nz.HipBackend(0)
        comm = b.local_comm(group, rank)
        try:
            ss = b.prover_session(cfg, max(LOGS))
            ss.set_comm(comm)
            try:
                results[rank] = _drive(ss, ap, lambda: ss.commit_host_narrow(wide, coset_order=True, as_kind=AS_KIND))
            finally:
                ss.close()
        except Exception as e:   # noqa: BLE001
            errors.append((rank, repr(e)))
            comm.abort(comm.user)
        finally:
            b.free_local_comm(comm)
            b.close()
    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    group.close()
    assert not errors and not any(t.is_alive() for t in th), errors
    for r in range(world):
        _same(one, results[r])


# ----------------------------------------------------------------------------------------------------------------------- 3. machine
def test_machine_narrow_preprocessed_columns_and_refusal(be, nz):
    comps = [(10, 3, 20, 8), (7, 2, 5, 4)]
    cfg = nz.default_config(pow_bits=5)
    ref = be.prove_machine(comps, cfg, seed=9, ad=b"narrow")
    pre = [c for s in be.synth_fill_tree(comps, 0, 9) for c in s.to_cpu()]
    main = [c for s in be.synth_fill_tree(comps, 1, 9) for c in s.to_cpu()]
    flags = [k < 2 for (_, n_pre, _, _) in comps for k in range(n_pre)]     # is_first / is_last of every component
    assert all(pre[i].max() <= 1 for i, f in enumerate(flags) if f)
    pre8 = [c.astype(np.uint8) if f else c for c, f in zip(pre, flags)]
    _same(ref, be.prove_machine_host_narrow(comps, cfg, pre8, main, ad=b"narrow"))
    _same(ref, be.prove_machine_host_narrow(comps, cfg, pre, main, ad=b"narrow", pre_as=[np.uint8 if f else None for f in flags]))
    # a full-field main column declared U32_AS_U16: refused, naming it; the same context then proves the right statement
    j = 22
    assert main[j].max() > 0xffff
    with pytest.raises(nz.NexusHipError) as e:
        be.prove_machine_host_narrow(comps, cfg, pre, main, ad=b"narrow", main_as=[np.uint16 if k == j else None for k in range(len(main))])
    msg = str(e.value)
    assert "main" in msg and re.search(r"column %d, row \d+" % j, msg) and "NX_COL_U32_AS_U16" in msg, msg
    _same(ref, be.prove_machine_host_narrow(comps, cfg, pre8, main, ad=b"narrow", pre_as=None))
