"""The trace checker (nx_air_check / nx_prover_check), the part that needs no GPU.

The judge of the checker is not the checker: `interp_check` below is a row-wise numpy interpreter of recorded programs over
NATURAL-order columns (the 15 opcodes, vectorised over the rows of the trace domain; a LOAD at offset o of row i reads row
(i + o) mod N).  The GPU tests compare the device's report with it exactly.  Here it is tied to the rest of the project: on
every valid statement the GPU tests use it reports nothing and the oracle's session proves that statement; on every tampered
one it reports something and the oracle's session refuses with ConstraintsNotSatisfied."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import air_examples as X
from test_prover_session_cpu import build_mixed_air

P = O.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ap():
    import nexus_zkvm_amd.air_program as ap
    return ap


# ---------------------------------------------------------------- the reference interpreter ----------------
def natural_row_of_pos(log_size):
    """row[pos]: the natural trace row (coset order) stored at position pos of the bit-reversed circle-domain order."""
    n = 1 << log_size
    pos = np.arange(n, dtype=np.int64)
    d = np.zeros(n, np.int64)
    for b in range(log_size):
        d |= ((pos >> b) & 1) << (log_size - 1 - b)
    return np.where(d < n // 2, 2 * d, 2 * n - 1 - 2 * d)


def to_natural(col):
    """A stored column (bit-reversed circle-domain order) in natural trace order."""
    col = np.asarray(col, np.uint64)
    out = np.zeros_like(col)
    out[natural_row_of_pos(int(np.log2(len(col))))] = col
    return out


def _cmul(a, b):
    return ((a[0] * b[0] + (P - (a[1] * b[1]) % P)) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _qmul(x, y):
    """QM31 = CM31[u] / (u^2 - 2 - i), coordinates as uint64 arrays"""
    aa, bb = _cmul(x[:2], y[:2]), _cmul(x[2:], y[2:])
    ab, ba = _cmul(x[:2], y[2:]), _cmul(x[2:], y[:2])
    r0, r1 = (2 * bb[0] + P - bb[1]) % P, (2 * bb[1] + bb[0]) % P
    return [(aa[0] + r0) % P, (aa[1] + r1) % P, (ab[0] + ba[0]) % P, (ab[1] + ba[1]) % P]


def interp_check(program, cols_nat, log_size, econsts=None):
    """{constraint: (n_rows, first_row, value at first_row)} of the constraints that are not zero somewhere.
    cols_nat: natural-order columns (None where the program loads nothing)."""
    ap = _ap()
    n = 1 << log_size
    ec = np.asarray(program.econsts if econsts is None else econsts, np.uint64).reshape(-1, 4)
    R = [np.zeros(n, np.uint64) for _ in range(program.n_regs + 4)]
    rows = np.arange(n)

    def load(c, off):
        return cols_nat[c][(rows + off) % n]

    def E(i):
        return R[i:i + 4]
    out, j = {}, 0
    for op, dst, a, b in np.asarray(program.instrs, np.uint32).reshape(-1, 4).tolist():
        if op == ap.LOAD:
            R[dst] = load(a, int(np.int32(np.uint32(b))))
        elif op == ap.CONST:
            R[dst] = np.full(n, a, np.uint64)
        elif op == ap.ADD:
            R[dst] = (R[a] + R[b]) % P
        elif op == ap.SUB:
            R[dst] = (R[a] + P - R[b]) % P
        elif op == ap.MUL:
            R[dst] = (R[a] * R[b]) % P
        elif op == ap.NEG:
            R[dst] = (P - R[a]) % P
        elif op == ap.CONSTE:
            R[dst:dst + 4] = [np.full(n, int(ec[a][k]), np.uint64) for k in range(4)]
        elif op == ap.ADDE:
            R[dst:dst + 4] = [(x + y) % P for x, y in zip(E(a), E(b))]
        elif op == ap.SUBE:
            R[dst:dst + 4] = [(x + P - y) % P for x, y in zip(E(a), E(b))]
        elif op == ap.MULE:
            R[dst:dst + 4] = _qmul(E(a), E(b))
        elif op == ap.MULEB:
            R[dst:dst + 4] = [(x * R[b]) % P for x in E(a)]
        elif op == ap.ADDEB:
            v = E(a)
            R[dst:dst + 4] = [(v[0] + R[b]) % P, v[1], v[2], v[3]]
        elif op == ap.LOADE:
            off = int(np.int32(np.uint32(b)))
            R[dst:dst + 4] = [load(a + k, off) for k in range(4)]
        elif op in (ap.CONSTRAINT_B, ap.CONSTRAINT_E):
            val = [R[a]] + ([R[a + 1], R[a + 2], R[a + 3]] if op == ap.CONSTRAINT_E else [np.zeros(n, np.uint64)] * 3)
            bad = np.nonzero(val[0] | val[1] | val[2] | val[3])[0]
            if len(bad):
                out[j] = (len(bad), int(bad[0]), tuple(int(v[bad[0]]) for v in val))
            j += 1
        else:
            raise AssertionError(f"opcode {op}")
    assert j == program.n_constraints
    return out


def expected_failures(components, trees):
    """The report of a statement: [(component, constraint, first_row, value, n_rows)] in (component, constraint) order.
    trees: the committed columns (stored order) per tree."""
    out = []
    for ci, c in enumerate(components):
        loaded = set()
        for op, _, a, _ in np.asarray(c.program.instrs, np.uint32).reshape(-1, 4).tolist():
            if op == _ap().LOAD:
                loaded.add(a)
            if op == _ap().LOADE:
                loaded.update(range(a, a + 4))
        cols = [to_natural(trees[t][i]) if k in loaded else None for k, (t, i) in enumerate(c.cols)]
        for j, (n_rows, first, val) in sorted(interp_check(c.program, cols, c.log_size).items()):
            out.append((ci, j, first, val, n_rows))
    return out


# ---------------------------------------------------------------- the statements of the GPU tests ----------
def drive_recording(sess, drive, hook=None, **kw):
    """Runs a build_mixed_air drive over a session and keeps what was committed: (components, trees).  hook(tree_index, cols)
    may change the columns of a tree before they are committed (the interaction trace is built from the untouched main trace)."""
    trees = []

    def commit(cols):
        cols = [np.array(c, np.uint32) for c in cols]
        if hook:
            hook(len(trees), cols)
        trees.append(cols)
        return sess.commit(cols)
    return drive(sess, commit, **kw), trees


def offsets_statement(ap, log=6, seed=5, tamper=None):
    """A component with offsets beyond +-1: columns a, b free, c with c[i] = a[i-3] * b[i+2] + a[i] (mask (-3, 0, 2))."""
    rng = np.random.default_rng(seed)
    n = 1 << log
    a, b = (rng.integers(0, P, n, dtype=np.uint64) for _ in range(2))
    c = (np.roll(a, 3) * np.roll(b, -2) + a) % P
    if tamper is not None:
        c[tamper] = (c[tamper] + 1) % P
    pb = ap.ProgramBuilder()
    am3, a0 = pb.next_trace_mask(0, (-3, 0))
    (b2,) = pb.next_trace_mask(1, (2,))
    (c0,) = pb.next_trace_mask(2)
    pb.add_constraint(c0 - am3 * b2 - a0)
    pb.add_constraint((c0 - a0) * 2 - am3 * b2 * 2)
    comp = ap.Component(log, pb.build(), [(0, 0), (0, 1), (0, 2)])
    return [[O.finalize_column(x.astype(np.uint32)) for x in (a, b, c)]], comp


MIXED = [dict(logs=(5, 7)), dict(logs=(6, 5), lcd=2, bounds=(2, 1), high_degree=True)]


def _oracle_proves(cfg, max_log, run):
    s = O.ProverSession(cfg, max_log)
    comps, trees = run(s)
    return s, comps, trees


@pytest.mark.parametrize("kw", MIXED)
def test_interpreter_agrees_with_the_oracle_session_on_the_logup_air(kw):
    lcd = kw.get("lcd", 1)
    cfg = O.default_cfg(pow_bits=2, log_constraint_degree=lcd, log_blowup=lcd)
    drive, _ = build_mixed_air(**kw)
    s = O.ProverSession(cfg, max(kw["logs"]))
    comps, trees = drive_recording(s, drive)
    assert expected_failures(comps, trees) == []            # every constraint, the [-1, 0] logup one across the wrap-around included
    s.prove(comps)
    s = O.ProverSession(cfg, max(kw["logs"]))
    comps, trees = drive_recording(s, drive, tamper="main")
    exp = expected_failures(comps, trees)
    row = 23 if kw["logs"][0] == 5 else 47                   # storage position 5 of main column c of component 0
    want = [0, 1, 2] if kw.get("high_degree") else [0]
    assert [(f[0], f[1], f[2], f[4]) for f in exp] == [(0, j, row, 1) for j in want]
    with pytest.raises(RuntimeError, match="ConstraintsNotSatisfied"):
        s.prove(comps)


@pytest.mark.parametrize("n_trees", [2, 3, 4])
def test_interpreter_agrees_with_the_oracle_session_on_the_synthetic_machine(n_trees):
    ap = _ap()
    cfg = O.default_cfg(pow_bits=3)
    trees, comp = X.tree_count_statement(ap, n_trees)
    assert expected_failures([comp], trees) == []            # offset +1 under the is_last selector
    s = O.ProverSession(cfg, comp.log_size)
    s.mix_u64(n_trees)
    for t in trees:
        s.commit(t)
    s.prove([comp])
    trees[1][5][9] = (int(trees[1][5][9]) + 1) % P
    assert expected_failures([comp], trees) != []
    s = O.ProverSession(cfg, comp.log_size)
    s.mix_u64(n_trees)
    for t in trees:
        s.commit(t)
    with pytest.raises(RuntimeError, match="ConstraintsNotSatisfied"):
        s.prove([comp])


def test_interpreter_on_offsets_beyond_one_and_the_row_numbering():
    ap = _ap()
    assert np.array_equal(to_natural(O.finalize_column(np.arange(64, dtype=np.uint32))), np.arange(64))   # the row formula is finalize_columns' inverse
    trees, comp = offsets_statement(ap)
    assert expected_failures([comp], trees) == []
    cfg = O.default_cfg(pow_bits=2)
    s = O.ProverSession(cfg, comp.log_size)
    s.commit(trees[0])
    s.prove([comp])
    trees, comp = offsets_statement(ap, tamper=0)           # c[0] reads a[N - 3] and b[2]: both wrap-arounds sit in one constraint
    exp = expected_failures([comp], trees)
    assert [(f[1], f[2], f[4]) for f in exp] == [(0, 0, 1), (1, 0, 1)] and exp[0][3] == (1, 0, 0, 0) and exp[1][3] == (2, 0, 0, 0)
    s = O.ProverSession(cfg, comp.log_size)
    s.commit(trees[0])
    with pytest.raises(RuntimeError, match="ConstraintsNotSatisfied"):
        s.prove([comp])


# ---------------------------------------------------------------- the generated source, the C ABI ----------
def test_check_source_tests_every_constraint_and_compiles_for_gfx950(tmp_path):
    import nexus_zkvm_amd as nz
    ap = _ap()
    comp = X.logup_component(ap, 6, (1, 2, 3, 4), (5, 6, 7, 8), (9, 1, 2, 3), high_degree=True)
    src = nz.air_check_source(comp.program, len(comp.cols))
    head = src[src.index('extern "C"'):]
    sig = head[:head.index("{")]
    assert "pw" not in sig and "denom_inv" not in sig and "count" in sig and "first" in sig
    body = head[head.index("{"):]
    assert body.count("CHECK(") == comp.program.n_constraints == 5
    assert all(f"CHECK({j}u, " in body for j in range(5))
    assert "pw[" not in body and "denom_inv" not in body and "q_mul(Q{pw" not in body and "a0[r]" not in body
    assert "trace_row_offset(r, log_size, -1)" in body and "row_offset(r, log_size, e" not in body
    # a many-constraint program is cut into several kernels, every constraint tested exactly once
    big = X.synthetic_component(ap, 6, 3, 200, 64)
    os.environ["NX_AIR_SEGMENT"] = "400"
    try:
        bsrc = nz.air_check_source(big.program, len(big.cols))
    finally:
        del os.environ["NX_AIR_SEGMENT"]
    assert bsrc.count('extern "C"') > 1
    assert bsrc.count("CHECK(") - 1 == big.program.n_constraints          # one is the macro's definition
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return
    for name, text in (("chk", src), ("chk_big", bsrc)):
        f = tmp_path / f"{name}.hip"
        f.write_text(text)
        subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-c", str(f), "-o", str(tmp_path / f"{name}.o")], check=True, timeout=300)


def test_check_argument_errors_are_codes_not_crashes():
    import nexus_zkvm_amd as nz
    ap = _ap()
    L = nz.load_library()
    comp = X.logup_component(ap, 6, (1, 2, 3, 4), (5, 6, 7, 8), (9, 1, 2, 3))
    ins = np.ascontiguousarray(comp.program.instrs, np.uint32).reshape(-1)
    ec = np.ascontiguousarray(comp.program.econsts, np.uint32).reshape(-1)
    n_i, n_r, n_c = len(ins) // 4, comp.program.n_regs, comp.program.n_constraints
    p_ins, p_ec = ins.ctypes.data_as(C.c_void_p), ec.ctypes.data_as(C.c_void_p)
    src = C.c_void_p()
    assert L.nx_air_check_source(None, n_i, n_r, 7, 3, n_c, C.byref(src)) == nz.NX_ERR_ARG
    assert L.nx_air_check_source(p_ins, n_i, n_r, 7, 3, n_c, None) == nz.NX_ERR_ARG
    assert L.nx_air_check_source(p_ins, n_i, n_r, 7, 3, n_c + 1, C.byref(src)) == nz.NX_ERR_ARG       # constraint count
    assert L.nx_air_check_source(p_ins, n_i, n_r, 6, 3, n_c, C.byref(src)) == nz.NX_ERR_ARG           # a LOADE beyond the columns
    assert L.nx_air_check_source(p_ins, n_i, n_r, 7, 2, n_c, C.byref(src)) == nz.NX_ERR_ARG           # a CONSTE beyond the constants
    assert L.nx_air_check_source(p_ins, n_i, 2, 7, 3, n_c, C.byref(src)) == nz.NX_ERR_ARG             # registers
    out = (nz.CheckFailureC * 4)()
    n = C.c_uint32(77)
    ptrs = (C.c_void_p * 7)()
    # no context: an error, and nothing is written
    assert L.nx_air_check(None, p_ins, n_i, n_r, ptrs, 7, p_ec, 3, n_c, 6, out, 4, C.byref(n)) == nz.NX_ERR_ARG and n.value == 77
    assert L.nx_air_check(None, p_ins, n_i, n_r, ptrs, 7, p_ec, 3, n_c, 6, out, 4, None) == nz.NX_ERR_ARG
    assert L.nx_air_check(None, p_ins, n_i, n_r, ptrs, 7, p_ec, 3, n_c, 6, None, 4, C.byref(n)) == nz.NX_ERR_ARG
    assert L.nx_prover_check(None, None, 0, out, 4, C.byref(n)) == nz.NX_ERR_ARG
    assert C.sizeof(nz.CheckFailureC) == 40


def test_header_with_the_checker_is_still_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    f = tmp_path / "h.c"
    f.write_text('#include "nexus_hip.h"\n'
                 'int f(nx_prover* p, const nx_air_component* c, nx_check_failure* o, uint32_t* n) { return nx_prover_check(p, c, 1, o, 4, n); }\n'
                 'int g(void) { return (int)sizeof(nx_check_failure); }\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(f), "-o", str(tmp_path / "h.o")], check=True)
