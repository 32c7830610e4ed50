"""The trace checker on the device: nx_air_check (one program over trace-domain columns) and nx_prover_check (the session form,
over the committed trees).  Every report is compared EXACTLY — failing constraints, row counts, first rows, values — with the numpy
interpreter of test_trace_check_cpu.py, which that file ties to the oracle's prover session.

test_check_time_against_the_prove prints the check / prove figures (-s); DESIGN.md section 7b holds what one MI355X gave."""
import ctypes as C
import os
import shutil
import statistics
import subprocess
import time

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import oracle_lib as O
import air_examples as X
from test_prover_session_cpu import build_mixed_air
from test_trace_check_cpu import expected_failures, drive_recording, offsets_statement, natural_row_of_pos, interp_check, to_natural

pytestmark = pytest.mark.gpu
P = O.P


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


@pytest.fixture(scope="module")
def ap():
    import nexus_zkvm_amd.air_program as ap
    return ap


def _hip_cfg(nz, ocfg):
    return nz.default_config(pow_bits=int(ocfg[0]), log_blowup=int(ocfg[1]), n_queries=int(ocfg[2]), log_last_layer_degree_bound=int(ocfg[3]),
                             hash_mode=int(ocfg[4]), fri_alpha_mode=int(ocfg[5]), log_constraint_degree=int(ocfg[6]))


def as_tuples(rep):
    return [(f.component, f.constraint, f.first_row, f.value, f.n_rows) for f in rep.failures]


def pos_of_row(log, row):
    return int(np.nonzero(natural_row_of_pos(log) == row)[0][0])


def mixed_session(be, nz, hook=None, tamper=None, **kw):
    lcd = kw.get("lcd", 1)
    ocfg = O.default_cfg(pow_bits=2, log_constraint_degree=lcd, log_blowup=lcd)
    drive, _ = build_mixed_air(**kw)
    s = be.prover_session(_hip_cfg(nz, ocfg), max(kw["logs"]))
    comps, trees = drive_recording(s, drive, hook=hook, **({"tamper": tamper} if tamper else {}))
    return s, comps, trees, ocfg, drive


def check_against_interpreter(s, comps, trees, max_failures=64):
    exp = expected_failures(comps, trees)
    rep = s.check(comps, max_failures=max_failures)
    assert rep.n_failed == len(exp) and rep.ok == (not exp)
    assert as_tuples(rep) == exp[:max_failures]
    if exp:
        c, j, row, _, n = exp[0]
        assert rep.message.endswith(f"component {c} constraint {j}: not zero on {n} of {1 << comps[c].log_size} rows, first at row {row}")
    return rep, exp


# ---------------------------------------------------------------- valid statements ----------------
@pytest.mark.parametrize("kw", [dict(logs=(5, 7)), dict(logs=(6, 5), lcd=2, bounds=(2, 1), high_degree=True),
                                dict(logs=(12, 8, 10), lcd=2, bounds=(1, 2, 1))])
def test_valid_logup_statements_pass(be, nz, kw):
    s, comps, trees, _, _ = mixed_session(be, nz, **kw)
    rep, exp = check_against_interpreter(s, comps, trees)
    assert rep.ok and rep.n_failed == 0 and rep.failures == [] and rep.message == ""
    s.close()


@pytest.mark.parametrize("n_trees", [2, 3, 4])
def test_valid_synthetic_machine_passes_with_any_tree_count(be, nz, ap, n_trees):
    """the recorded synthetic machine: offset +1 under the is_last selector"""
    trees, comp = X.tree_count_statement(ap, n_trees)
    s = be.prover_session(nz.default_config(pow_bits=3), comp.log_size)
    s.mix_u64(n_trees)
    for t in trees:
        s.commit(t)
    assert check_against_interpreter(s, [comp], trees)[0].ok
    s.close()


@pytest.mark.parametrize("tamper", [None, 0, 63, 17])
def test_offsets_beyond_one(be, nz, ap, tamper):
    """mask (-3, 0, 2): valid, and one cell wrong at row 0 / N - 1 (both wrap-arounds) / in the middle"""
    trees, comp = offsets_statement(ap, tamper=tamper)
    s = be.prover_session(nz.default_config(pow_bits=2), comp.log_size)
    s.commit(trees[0])
    rep, exp = check_against_interpreter(s, [comp], trees)
    assert rep.ok == (tamper is None)
    if tamper is not None:
        assert [(f.constraint, f.first_row, f.n_rows, f.value) for f in rep.failures] == [(0, tamper, 1, (1, 0, 0, 0)), (1, tamper, 1, (2, 0, 0, 0))]
    s.close()


# ---------------------------------------------------------------- tampered statements ----------------
def test_one_cell_of_a_main_column(be, nz):
    for kw, row, cons in ((dict(logs=(5, 7)), 23, [0]), (dict(logs=(6, 5), lcd=2, bounds=(2, 1), high_degree=True), 47, [0, 1, 2])):
        s, comps, trees, _, _ = mixed_session(be, nz, tamper="main", **kw)
        rep, exp = check_against_interpreter(s, comps, trees)
        assert [(f.component, f.constraint, f.first_row, f.n_rows) for f in rep.failures] == [(0, j, row, 1) for j in cons]
        s.close()


@pytest.mark.parametrize("row", [0, 31])
def test_a_main_cell_at_the_first_and_the_last_row(be, nz, row):
    def hook(t, cols):
        if t == 1:
            cols[0][pos_of_row(5, row)] ^= 1          # a of component 0: c - a b - 3 and the logup denominator at that row
    s, comps, trees, _, _ = mixed_session(be, nz, hook=hook, logs=(5, 7))
    rep, exp = check_against_interpreter(s, comps, trees)
    assert [(f.component, f.constraint, f.first_row, f.n_rows) for f in rep.failures] == [(0, 0, row, 1), (0, 1, row, 1)]
    s.close()


@pytest.mark.parametrize("row,rows", [(0, (0, 1)), (31, (0, 31)), (12, (12, 13))])
def test_one_coordinate_of_the_secure_column_fails_two_rows(be, nz, row, rows):
    """S(row) enters the [-1, 0] constraint at row and at row + 1 — row N - 1 wraps to row 0, row 0 is read from row 1"""
    def hook(t, cols):
        if t == 2:
            cols[2][pos_of_row(5, row)] = (int(cols[2][pos_of_row(5, row)]) + 5) % P
    s, comps, trees, _, _ = mixed_session(be, nz, hook=hook, logs=(5, 7))
    rep, exp = check_against_interpreter(s, comps, trees)
    assert [(f.component, f.constraint, f.first_row, f.n_rows) for f in rep.failures] == [(0, 1, min(rows), 2)]
    assert any(rep.failures[0].value[1:])          # a secure value: not only the first coordinate
    s.close()


def test_a_zeroed_column_fails_every_row_of_several_constraints(be, nz):
    def hook(t, cols):
        if t == 1:
            cols[3 + 1][:] = 0                         # b of component 1 (2^7 rows)
    s, comps, trees, _, _ = mixed_session(be, nz, hook=hook, logs=(5, 7))
    rep, exp = check_against_interpreter(s, comps, trees)
    assert [(f.component, f.constraint) for f in rep.failures] == [(1, 0), (1, 1)] and all(f.n_rows >= 127 for f in rep.failures)
    s.close()


def test_two_components_at_once_and_a_small_cap(be, nz):
    def hook(t, cols):
        if t == 1:
            cols[2][9] ^= 4                            # c of component 0
            cols[3 + 0][20] ^= 2                       # a of component 1
    kw = dict(logs=(6, 5), lcd=2, bounds=(2, 1), high_degree=True)
    s, comps, trees, _, _ = mixed_session(be, nz, hook=hook, **kw)
    rep, exp = check_against_interpreter(s, comps, trees)
    assert [(f.component, f.constraint) for f in rep.failures] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
    for cap in (0, 1, 4):
        small, _ = check_against_interpreter(s, comps, trees, max_failures=cap)
        assert small.n_failed == 5 and len(small.failures) == cap
    s.close()


def test_a_wrong_lookup_element_fails_the_logup_constraint_everywhere(be, nz, ap):
    s, comps, trees, _, _ = mixed_session(be, nz, logs=(5, 7))
    pr = comps[1].program
    ec = np.array(pr.econsts, np.uint32).copy()
    ec[0][0] ^= 1
    bad = ap.Component(comps[1].log_size, ap.Program(pr.instrs, pr.n_regs, ec, pr.n_constraints, pr.masks), comps[1].cols, comps[1].masks)
    rep, exp = check_against_interpreter(s, [comps[0], bad], trees)
    assert [(f.component, f.constraint) for f in rep.failures] == [(1, 1)] and rep.failures[0].n_rows >= 127 and rep.failures[0].first_row == 0
    assert s.check(comps).ok                           # the statement itself is fine
    s.close()


# ---------------------------------------------------------------- the primitive, the transform under the session form ----------------
def test_forward_transform_without_expansion_undoes_the_interpolation(be):
    """nx_prover_check evaluates committed coefficients on the trace domain with log_expand 0 — a value no other caller passes"""
    for log in (1, 2, 5, 9, 12, 13, 15):
        vals = np.random.default_rng(log).integers(0, P, (3, 1 << log), dtype=np.uint32)
        tw = be.precompute_twiddles(max(log - 1, 1) + 2)
        cols = be.columns_from_host(vals)
        be.interpolate_columns(tw, cols)
        back = be.evaluate_polynomials(tw, cols, 0)
        assert np.array_equal(back.to_cpu(), vals), log


def test_the_primitive_on_uncommitted_columns_gives_the_session_report(be, nz):
    def hook(t, cols):
        if t == 1:
            cols[1][3] ^= 8
        if t == 2:
            cols[0][7] ^= 1
    s, comps, trees, _, _ = mixed_session(be, nz, hook=hook, logs=(5, 7))
    rep = s.check(comps)
    assert not rep.ok
    c0 = comps[0]
    dev = [be.columns_from_host(trees[t][i]) for t, i in c0.cols]
    ptrs = [d.ptr.value for d in dev]
    prim = be.air_check(c0.program, ptrs, c0.log_size)
    assert as_tuples(prim) == [f for f in as_tuples(rep) if f[0] == 0] and prim.n_failed == rep.n_failed and prim.message == rep.message
    ptrs[7] = None                                     # the preprocessed column no constraint loads
    assert as_tuples(be.air_check(c0.program, ptrs, c0.log_size)) == as_tuples(prim)
    ptrs[1] = None
    with pytest.raises(nz.NexusHipError, match="passed as NULL"):
        be.air_check(c0.program, ptrs, c0.log_size)
    with pytest.raises(nz.NexusHipError, match="log_size"):
        be.air_check(c0.program, [d.ptr.value for d in dev], 0)
    s.close()


def test_the_garbage_trace_recipe_fails_what_it_is_meant_to(be, ap):
    """the worst case of the reporting path, as test_check_time_against_the_prove measures it: every derived main column overwritten
    with a free random column of its group.  At a small size, against the interpreter."""
    comps = [(6, 3, 40, 8)]
    comp = X.synthetic_component(ap, *comps[0])
    trees = [O.synth_tree_columns(comps, 0, 4), O.synth_tree_columns(comps, 1, 4), O.synth_tree_columns(comps, 2, 4, 9)]
    assert expected_failures([comp], trees) == []
    for k in range(40):
        if k % 16 >= 2:
            trees[1][k] = trees[1][(k // 16) * 16].copy()
    exp = expected_failures([comp], trees)
    n_main_constraints = sum(1 for k in range(2, 40) if k % 16 >= 2)
    assert len([f for f in exp if f[4] >= 60]) >= n_main_constraints - 2          # nearly every row of nearly every main constraint
    dev = [be.columns_from_host(trees[t][i]) for t, i in comp.cols]
    rep = be.air_check(comp.program, [d.ptr.value for d in dev], 6, max_failures=256)
    assert as_tuples(rep) == exp


# ---------------------------------------------------------------- the session is left alone ----------------
def test_check_leaves_the_transcript_and_the_proof_alone(be, nz, oracle):
    kw = dict(logs=(10, 8), lcd=2, bounds=(2, 1), high_degree=True)
    s, comps, trees, ocfg, drive = mixed_session(be, nz, **kw)
    so = oracle.ProverSession(ocfg, 10)
    ref = so.prove(drive(so, so.commit))
    d0 = s.digest()
    assert s.check(comps).ok and np.array_equal(s.digest(), d0)
    words = s.prove(comps)
    assert np.array_equal(words, ref)
    d1 = s.digest()
    assert s.check(comps).ok and np.array_equal(s.digest(), d1)          # after the prove: the composition tree is not part of the statement
    assert np.array_equal(s.prove(comps), ref)
    s.close()


def test_a_refused_trace_is_reported_and_the_session_stays_usable(be, nz):
    s, comps, trees, _, _ = mixed_session(be, nz, tamper="main", logs=(5, 7))
    d0 = s.digest()
    rep = s.check(comps)
    assert not rep.ok and rep.failures[0][:3] == (0, 0, 23)
    with pytest.raises(nz.NexusHipError, match="ConstraintsNotSatisfied"):
        s.prove(comps)
    assert np.array_equal(s.digest(), d0)
    assert as_tuples(s.check(comps)) == as_tuples(rep)
    with pytest.raises(nz.NexusHipError, match="ConstraintsNotSatisfied"):
        s.prove(comps)
    s.close()


def test_statement_errors_are_the_provers(be, nz, ap):
    s, comps, trees, _, _ = mixed_session(be, nz, logs=(5,))
    c0 = comps[0]
    for bad, text in (([ap.Component(c0.log_size, c0.program, c0.cols[:-1], c0.masks[:-1])], "claimed by no component"),
                      ([ap.Component(c0.log_size, c0.program, c0.cols, [[0]] * len(c0.cols))], "missing from the column's mask"),
                      ([ap.Component(c0.log_size, c0.program, [(5, 0)] + c0.cols[1:], c0.masks)], "outside the committed trees")):
        with pytest.raises(nz.NexusHipError, match=text) as e1:
            s.check(bad)
        with pytest.raises(nz.NexusHipError, match=text) as e2:
            s.prove(bad)
        assert str(e1.value) == str(e2.value)
    assert s.check(comps).ok
    s.close()


def test_a_session_with_a_communicator_is_refused(nz, ap):
    """checking a row-sharded trace is out of scope: NX_ERR_ARG before anything else happens"""
    from nexus_zkvm_amd import _air_components
    b = nz.HipBackend(0)
    group = nz.LocalGroup(2)
    comm = b.local_comm(group, 0)
    s = b.prover_session(nz.default_config(pow_bits=2), 6)
    s.set_comm(comm)
    _, comp = offsets_statement(ap)
    with pytest.raises(nz.NexusHipError, match="one GPU"):
        s.check([comp])
    out, n = (nz.CheckFailureC * 1)(), C.c_uint32(0)
    arr, keep = _air_components([comp])
    assert b.L.nx_prover_check(s.h, arr, 1, out, 1, C.byref(n)) == nz.NX_ERR_ARG
    s.close(); b.free_local_comm(comm); b.close(); group.close()


def test_c_example_names_the_constraint_and_the_row_it_corrupts(tmp_path):
    """examples/session_prove.c with the `check` argument: storage position 7 of column c is natural row 15 of the 2^6-row trace.
    Without the argument its output is what it was (tests/test_gpu_verifier.py, tests/test_gpu_parity.py pin it)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(root, "nexus-zkvm_amd")
    exe = str(tmp_path / "session_prove")
    subprocess.run([shutil.which("gcc"), "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "session_prove.c"),
                    "-L" + lib_dir, "-lnexus_hip", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    out = subprocess.run([exe, "bad", "check"], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0] == "check: component 0 constraint 0: 1 row(s), first at row 15, value 1"
    assert out[1].startswith("refused:") and "ConstraintsNotSatisfied" in out[1] and len(out) == 2
    out = subprocess.run([exe, "check"], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0] == "check: ok" and out[1].startswith("ok ") and out[2] == "verified: accepted" and len(out) == 4


# ---------------------------------------------------------------- memory, kernel reuse ----------------
def test_memory_stays_within_the_stated_bound_and_nothing_leaks(be, nz, ap):
    """include/nexus_hip.h: peak above the session's <= 4 * 2^log_size * (columns the constraints load) of the largest component
    + 24 bytes per column and constraint (+ 20 bytes per loaded word of every distinct reported first row on the failing path), each
    term rounded up to 256."""
    def loaded(c):
        cols, words = set(), 0
        for op, _, a, _ in np.asarray(c.program.instrs, np.uint32).reshape(-1, 4).tolist():
            if op == ap.LOAD:
                cols.add(a); words += 1
            if op == ap.LOADE:
                cols.update(range(a, a + 4)); words += 4
        return len(cols), words

    def up(x):
        return (x + 255) // 256 * 256
    for tamper in (None, "main"):
        s, comps, trees, _, _ = mixed_session(be, nz, tamper=tamper, logs=(12, 8, 10), lcd=2, bounds=(1, 2, 1))
        s.check(comps)                                  # compiles; the measured call below is steady state
        be.sync()
        live0, _ = be.memory(reset_peak=True)
        rep = s.check(comps)
        live1, peak = be.memory()
        assert rep.ok == (tamper is None)
        assert live1 == live0
        bound = max(up(4 * (1 << c.log_size) * loaded(c)[0]) + up(24 * (len(c.cols) + c.program.n_constraints)) +
                    (up(20 * loaded(c)[1] * len({f.first_row for f in rep.failures if f.component == i})) if not rep.ok else 0)
                    for i, c in enumerate(comps))
        assert 4 * (1 << 12) * 7 <= peak - live0 <= bound, (peak - live0, bound)
        s.close()


def test_check_kernels_are_compiled_once_per_program(be, nz, ap):
    trees, comp = offsets_statement(ap, log=7, seed=77)
    s = be.prover_session(nz.default_config(pow_bits=2), 7)
    s.commit(trees[0])
    assert s.check([comp]).ok
    before = nz.air_cache_stats()
    assert s.check([comp]).ok
    dev = be.columns_from_host(np.stack(trees[0]))
    assert be.air_check(comp.program, [dev.ptr.value + k * (4 << 7) for k in range(3)], 7).ok      # the same program through the primitive
    assert nz.air_cache_stats() == before
    s.close()


# ---------------------------------------------------------------- measurements ----------------
def _median_ms(fn, be, n=5):
    fn(); be.sync()
    ts = []
    for _ in range(n):
        be.sync(); t0 = time.perf_counter(); fn(); be.sync(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def test_check_time_against_the_prove(be, nz, ap):
    """The bench's column shape (27 + 347 + 64 columns, 436 base-field constraints, one +1 offset) at 2^20 rows as the recorded synthetic
    machine, traces filled on the device.  Prints (-s): the primitive on the filled columns, the session form (with its N-point
    transforms), nx_prover_prove of the same session and its composition stage; then the primitive on a garbage main tree (nearly
    every constraint fails on nearly every row: the worst case of the reporting path).  No thresholds beyond sanity: the figures go
    to DESIGN.md section 7b.  One MI355X gave: nx_air_check 0.43 ms, nx_prover_check 2.23 ms, nx_prover_prove 3.70 ms (composition
    0.55 ms), garbage main tree 0.71 ms (16.9 ms before the per-block LDS stage of the reporting path)."""
    from test_air_program_cpu import synthetic_program
    log, n_pre, n_main, n_inter = 20, 27, 347, 64
    comps = [(log, n_pre, n_main, n_inter)]
    cfg = nz.default_config()
    cols = [(0, k) for k in range(n_pre)] + [(1, k) for k in range(n_main)] + [(2, k) for k in range(n_inter)]
    comp = ap.Component(log, synthetic_program(ap, n_pre, n_main, n_inter), cols)
    carr = be._comps(comps)
    s = be.prover_session(cfg, log)

    def fill_into(ptrs, tree, inter_seed=0):
        be._chk(be.L.nx_synth_fill_tree(be.ctx, carr, 1, tree, C.c_uint64(1), C.c_uint64(inter_seed), (C.c_void_p * len(ptrs))(*ptrs)))

    def fill(tree, n, inter_seed=0):
        fill_into(s.tree_begin([log] * n), tree, inter_seed)
        return s.tree_commit()
    s.mix_u64(log)
    fill(0, n_pre); fill(1, n_main)
    z = s.draw_felt()
    s.mix_felts(np.zeros(4, np.uint32))
    inter_seed = (int(z[0]) << 32) ^ int(z[1]) ^ (int(z[2]) << 16) ^ (int(z[3]) << 48)
    fill(2, n_inter, inter_seed)
    # the same values in columns of our own: what a caller holds before the commit
    own = [be.columns(n, log) for n in (n_pre, n_main, n_inter)]
    for t, d in enumerate(own):
        fill_into([d.ptr.value + k * (4 << log) for k in range(d.n_cols)], t, inter_seed if t == 2 else 0)
    ptrs = [own[t].ptr.value + k * (4 << log) for t, k in cols]
    rep = be.air_check(comp.program, ptrs, log)
    assert rep.ok
    t_prim = _median_ms(lambda: be.air_check(comp.program, ptrs, log), be, n=21)
    assert s.check([comp]).ok
    t_sess = _median_ms(lambda: s.check([comp]), be, n=7)
    s.prove([comp])
    runs = [s.prove([comp], want_stats=True)[1] for _ in range(7)]
    t_prove = statistics.median(r["total"] for r in runs)
    t_comp = statistics.median(r["composition"] for r in runs)
    # garbage main tree: every derived column becomes a copy of its group's first free column
    for k in range(n_main):
        if k % 16 >= 2:
            be._chk(be.L.nx_copy(be.ctx, C.c_void_p(own[1].ptr.value + k * (4 << log)), C.c_void_p(own[1].ptr.value + (k // 16) * 16 * (4 << log)), C.c_size_t(1 << log)))
    bad = be.air_check(comp.program, ptrs, log, max_failures=8)
    n_all_rows = sum(1 for f in be.air_check(comp.program, ptrs, log, max_failures=512).failures if f.n_rows > (1 << log) * 0.99)
    t_bad = _median_ms(lambda: be.air_check(comp.program, ptrs, log, max_failures=8), be, n=21)
    print(f"\ntrace check at 2^{log} rows, {n_pre}+{n_main}+{n_inter} columns, {comp.program.n_constraints} constraints: "
          f"nx_air_check {t_prim:.2f} ms, nx_prover_check {t_sess:.2f} ms, nx_prover_prove {t_prove:.2f} ms (composition {t_comp:.2f} ms); "
          f"garbage main tree: {bad.n_failed} constraints fail ({n_all_rows} on > 99 % of the rows), nx_air_check {t_bad:.2f} ms")
    assert not bad.ok and bad.n_failed > 300 and n_all_rows > 280
    assert t_prim > 0 and t_sess > 0 and t_prove > 0
    s.close()
