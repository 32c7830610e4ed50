"""nx_trace_program, what needs no GPU: the export and its bindings, every refusal through the source-only form with a NULL context,
the other program kinds refusing the NX_T_* opcodes, the generated text (cross-compiled for gfx950; cut into segments) — and the text
itself run on the host under the address and undefined-behaviour sanitizers (tests/native/trace_text_host.cpp) against the numpy
interpreter of tests/trace_programs.py, word for word."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import trace_programs as TP
from test_air_text_host_cpu import _clangxx
from test_rust_shim_cpu import header_functions, rust_extern_functions

P = TP.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "native", "trace_text_host.cpp")
NX_ERR_ARG = -2
(LOAD, CONST, ADD, SUB, MUL, NEG, CONSTE, ADDE, SUBE, MULE, MULEB, ADDEB, LOADE, CONSTRAINT_B, CONSTRAINT_E, FRAC, FRACB) = range(17)
(STORE, STORE_IF, ROW, AND, OR, XOR, SHL, SHR, LTU, EQ, INV) = range(32, 43)


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    nexus_zkvm_amd.load_library()
    return nexus_zkvm_amd


def _call(nz, instrs, n_regs, n_cols, ptrs=None, log_size=5, want_source=True):
    """nx_trace_program with a NULL context: (code, nx_last_error, source or None).  ptrs: host-side numbers that are never followed."""
    L = nz.load_library()
    f = L.nx_trace_program
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    ins = np.ascontiguousarray(np.asarray(instrs, dtype=np.int64).astype(np.uint32).reshape(-1)) if instrs is not None else None
    table = (C.c_void_p * len(ptrs))(*ptrs) if ptrs is not None else None
    src = C.c_void_p()
    rc = f(None, ins.ctypes.data_as(C.c_void_p) if ins is not None else None, 0 if ins is None else len(ins) // 4, n_regs, table, n_cols, log_size,
           C.byref(src) if want_source else None)
    text = None
    if src.value:
        text = C.string_at(src.value).decode()
        L.nx_free_host(src)
    return rc, L.nx_last_error(None).decode(), text


GOOD = [(LOAD, 0, 0, 0), (CONST, 1, 5, 0), (XOR, 1, 0, 1), (STORE, 0, 1, 1)]


# ---------------------------------------------------------------- the export, the bindings, the header ----------
def test_symbol_is_declared_exported_and_bound(nz):
    assert "nx_trace_program" in nz.declared_symbols() and hasattr(nz.load_library(), "nx_trace_program")
    assert hasattr(nz.HipBackend, "trace_program") and hasattr(nz, "trace_program_source")
    h, r = header_functions(), rust_extern_functions()
    assert h["nx_trace_program"] == 8 == r["nx_trace_program"]
    chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert chk.returncode == 0, chk.stdout + chk.stderr
    sys_src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    assert "pub fn nx_trace_program(ctx: *mut nx_ctx, program: *const nx_cinstr," in sys_src
    hip = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "trace_program.rs")).read()
    assert "pub struct TraceProgram" in hip and "pub fn trace_program(&mut self" in hip and "sys::nx_trace_program(" in hip
    # the opcode numbers: header, Python recorder, Rust builder
    import nexus_zkvm_amd.air_program as ap
    header = open(nz.HEADER_PATH).read()
    names = ("STORE", "STORE_IF", "ROW", "AND", "OR", "XOR", "SHL", "SHR", "LTU", "EQ", "INV")
    for k, name in enumerate(names):
        assert re.search(r"\bNX_T_%s = %d\b" % (name, 32 + k), header), name
        assert getattr(ap, "T_" + name) == 32 + k
        assert "pub const NX_T_%s: u32 = %d;" % (name, 32 + k) in sys_src and "sys::NX_T_%s," % name in hip, name
    assert len(set(re.findall(r"\b(NX_C_[A-Z_]+)\b\s*=", header))) == 17          # the constraint opcodes are what they were


def test_header_with_the_trace_opcodes_is_still_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    f = tmp_path / "h.c"
    f.write_text('#include "nexus_hip.h"\n'
                 'int f(nx_ctx* c, const nx_cinstr* p, uint32_t* const* cols, char** s) { return nx_trace_program(c, p, 4, 2, cols, 3, 8, s); }\n'
                 'int g(void) { return NX_T_STORE + NX_T_STORE_IF + NX_T_ROW + NX_T_AND + NX_T_OR + NX_T_XOR + NX_T_SHL + NX_T_SHR + NX_T_LTU + NX_T_EQ + NX_T_INV; }\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(f), "-o", str(tmp_path / "h.o")], check=True)


# ---------------------------------------------------------------- refusals ----------
def refusal_cases():
    """(name, instrs, n_regs, n_cols, ptrs, log_size, the instruction nx_last_error must name or None) — shared with the GPU suite,
    which runs them through a live context (ptrs None: the caller's own device columns)."""
    two = [0x1000, 0x2000]
    return [
        ("secure constant", [(CONSTE, 0, 0, 0)] + GOOD, 4, 2, None, 5, 0),
        ("secure load", GOOD[:3] + [(LOADE, 0, 0, 0), GOOD[3]], 4, 4, None, 5, 3),
        ("secure product", GOOD[:3] + [(MULEB, 0, 0, 1), GOOD[3]], 8, 2, None, 5, 3),
        ("constraint", GOOD + [(CONSTRAINT_B, 0, 1, 0)], 2, 2, None, 5, 4),
        ("secure constraint", GOOD + [(CONSTRAINT_E, 0, 0, 0)], 4, 2, None, 5, 4),
        ("fraction", GOOD + [(FRACB, 0, 1, 0)], 4, 2, None, 5, 4),
        ("unknown opcode", GOOD + [(17, 0, 0, 0)], 2, 2, None, 5, 4),
        ("no store", GOOD[:3], 2, 2, None, 5, None),
        ("read before write", [(LOAD, 0, 0, 0), (ADD, 1, 0, 1), (STORE, 0, 1, 1)], 2, 2, None, 5, 1),
        ("store of an unwritten register", [(LOAD, 0, 0, 0), (STORE, 0, 1, 1)], 2, 2, None, 5, 1),
        ("flag never written", [(LOAD, 0, 0, 0), (STORE_IF, 1, 1, 0)], 2, 2, None, 5, 1),
        ("load of a stored column", [(LOAD, 0, 1, 1)] + GOOD[1:], 2, 2, None, 5, 0),
        ("load of a column stored later, other offset", GOOD + [(LOAD, 0, 2, 0xFFFFFFFE), (STORE, 0, 2, 1)], 2, 3, None, 5, 4),
        ("register out of range", [(LOAD, 2, 0, 0)] + GOOD[1:], 2, 2, None, 5, 0),
        ("operand register out of range", GOOD[:2] + [(XOR, 1, 0, 2), GOOD[3]], 2, 2, None, 5, 2),
        ("loaded column out of range", [(LOAD, 0, 2, 0)] + GOOD[1:], 2, 2, None, 5, 0),
        ("stored column out of range", GOOD[:3] + [(STORE, 0, 2, 1)], 2, 2, None, 5, 3),
        ("immediate not below p", [GOOD[0], (CONST, 1, P, 0)] + GOOD[2:], 2, 2, None, 5, 1),
        ("store with a dst", GOOD[:3] + [(STORE, 1, 1, 1)], 2, 2, None, 5, 3),
        ("no registers", GOOD, 0, 2, None, 5, None),
        ("too many registers", GOOD, 4097, 2, None, 5, None),
        ("log_size 0", GOOD, 2, 2, None, 0, None),
        ("log_size 31", GOOD, 2, 2, None, 31, None),
        ("loaded column NULL", GOOD, 2, 2, [None, 0x2000], 5, 0),
        ("stored column NULL", GOOD, 2, 2, [0x1000, None], 5, 3),
        ("output shares a pointer with an input", GOOD, 2, 2, [0x1000, 0x1000], 5, 3),
        ("output shares a pointer with an unused entry", GOOD, 2, 3, two + [0x2000], 5, 3),
    ]


@pytest.mark.parametrize("case", refusal_cases(), ids=lambda c: c[0])
def test_refusals_with_a_null_context(nz, case):
    _, instrs, n_regs, n_cols, ptrs, log_size, named = case
    rc, msg, text = _call(nz, instrs, n_regs, n_cols, ptrs, log_size)
    assert rc == NX_ERR_ARG and text is None, (rc, msg)
    if named is not None:
        assert f"instruction {named}:" in msg, msg


def test_null_arguments_are_codes_not_crashes(nz):
    rc, msg, text = _call(nz, GOOD, 2, 2)
    assert rc == 0 and "o1[3] = r1;" in text and "GW4(cols[1])[q] = o1;" in text      # the source-only form: no context, no column table
    rc, _, text = _call(nz, GOOD, 2, 2, [0x1000, 0x2000])                   # a table of numbers that are never followed
    assert rc == 0 and text
    assert _call(nz, None, 2, 2)[0] == NX_ERR_ARG                           # no program
    rc, msg, _ = _call(nz, GOOD, 2, 2, want_source=False)                   # nothing wanted: running needs a context
    assert rc == NX_ERR_ARG and "context" in msg
    rc, msg, _ = _call(nz, GOOD, 2, 2, [0x1000, 0x2000], want_source=False)
    assert rc == NX_ERR_ARG and "context" in msg
    assert _call(nz, [], 2, 2)[0] == NX_ERR_ARG                             # an empty program has no store


def test_the_other_program_kinds_refuse_the_trace_opcodes(nz):
    """validate_air_program / validate_logup_program: constraint, fraction and check entry points, every NX_T_* opcode"""
    L = nz.load_library()
    for op in range(32, 43):
        cons = np.array([(LOAD, 0, 0, 0), (op, 0 if op == STORE else 1, 0, 0), (CONSTRAINT_B, 0, 0, 0)], np.uint32).reshape(-1)
        p = cons.ctypes.data_as(C.c_void_p)
        src = C.c_void_p()
        assert L.nx_air_compile(None, p, 3, 2, 2, 0, 1, None, C.byref(src)) == NX_ERR_ARG and not src.value
        assert b"malformed instruction 1" in L.nx_last_error(None)
        assert L.nx_air_check_source(p, 3, 2, 2, 0, 1, C.byref(src)) == NX_ERR_ARG and not src.value
        deg = (C.c_uint32 * 1)()
        assert L.nx_air_constraint_degrees(None, p, 3, 2, 2, 0, 1, deg) == NX_ERR_ARG
        out, n = (nz.CheckFailureC * 1)(), C.c_uint32(7)
        assert L.nx_air_check(None, p, 3, 2, (C.c_void_p * 2)(), 2, None, 0, 1, 5, out, 1, C.byref(n)) == NX_ERR_ARG and n.value == 7
        frac = np.array([(LOAD, 0, 0, 0), (CONSTE, 4, 0, 0), (op, 0 if op == STORE else 1, 0, 0), (FRACB, 0, 0, 4)], np.uint32).reshape(-1)
        ec = np.zeros(4, np.uint32)
        csrc = C.c_char_p()
        assert L.nx_logup_program(None, frac.ctypes.data_as(C.c_void_p), 4, 8, None, 2, ec.ctypes.data_as(C.c_void_p), 1, 5, 1, None, C.byref(csrc)) == NX_ERR_ARG
        assert b"malformed instruction 2" in L.nx_last_error(None)


# ---------------------------------------------------------------- the generated text ----------
def _stores_per_column(text, n_cols, vec4):
    """per column: the store statements of the text (four positions per lane: the statements of the lane's first position)"""
    pat = r"\bo%d\[0\] = " if vec4 else r"GW\(cols\[%d\]\)\[r\] = "
    return [len(re.findall(pat % k, text)) for k in range(n_cols)]


@pytest.mark.parametrize("vec4", [0, 1])
def test_generated_text_shape_segments_and_gfx950_compilation(nz, tmp_path, monkeypatch, vec4):
    """both kernel shapes (NX_TRACE_VEC4 seeds the context option "trace.vec4"; without a context it decides): one row per lane, and
    four storage positions per lane for programs whose loads all have offset 0"""
    monkeypatch.setenv("NX_TRACE_VEC4", str(vec4))
    prog, n_cols, n_in = TP.opcode_table()
    text = nz.trace_program_source(prog, n_cols)
    assert text.count('extern "C"') == 1
    sig = text[text.index('extern "C"'):]
    sig = sig[:sig.index("{")]
    assert "econst" not in sig and "pw" not in sig and "u32* const* __restrict__ cols, int log_size, u32 n" in sig
    assert _stores_per_column(text, n_cols, vec4) == [0] * n_in + [1] * (n_cols - n_in)
    assert "const u32 nat" not in text                                       # no ROW: the natural row is not derived
    if vec4:
        assert "if (q >= n / 4) return;" in text and text.count("GW4(cols[") == n_cols - n_in and "G4(cols[0])[q]" in text and "GW(cols[" not in text
    else:
        assert "if (r >= n) return;" in text and "GW4(cols[" not in text.split('extern "C"')[1]
    # offsets: always one row per lane
    off, n_off, _ = TP.offsets_program()
    otext = nz.trace_program_source(off, n_off)
    for o in ("-2", "-1", "1", "3"):
        assert f"trace_row_offset(r, log_size, {o})" in otext
    assert "const u32 nat = coset_row_of_pos(r, log_size);" in otext and "row_offset(r, log_size, e" not in otext and "if (r >= n) return;" in otext
    # a small budget: several kernels, every store in exactly one of them
    monkeypatch.setenv("NX_AIR_SEGMENT", "200")
    stext = nz.trace_program_source(prog, n_cols)
    monkeypatch.delenv("NX_AIR_SEGMENT")
    kernels = stext.split('extern "C"')[1:]
    assert len(kernels) > 1 and len(prog.instrs[prog.instrs[:, 0] == STORE]) >= 40
    assert _stores_per_column(stext, n_cols, vec4) == [0] * n_in + [1] * (n_cols - n_in)
    assert all("GW4(cols[" in k if vec4 else "GW(cols[" in k for k in kernels)
    sif, n_sif, _ = TP.store_if_program()
    stt = nz.trace_program_source(sif, n_sif)
    assert _stores_per_column(stt, n_sif, vec4) == [0, 0, 0, 0, 0, 4]
    assert ("v4u o5 = G4(cols[5])[q];" in stt) == bool(vec4)                  # a column written under a flag starts from its stored words
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return
    for name, t in (("table", text), ("table_seg", stext), ("store_if", stt)) + ((("offsets", otext),) if not vec4 else ()):
        f = tmp_path / f"{name}.hip"
        f.write_text(t)
        subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-c", str(f), "-o", str(tmp_path / f"{name}.o")], check=True, timeout=300)


# ---------------------------------------------------------------- the host twin ----------
def _run_twin(tmp_path, name, text, cases):
    """Builds the driver around the text with the sanitizers and runs it once per (log_size, columns before, columns after), stored order."""
    clangxx = _clangxx()
    (tmp_path / f"{name}.hip").write_text(text)
    kernels = re.findall(r'extern "C" __attribute__\(\(global\)\)[^\n]*? void (\w+)\(', text)
    assert kernels and kernels[0] == "air_kernel"
    exe = str(tmp_path / name)
    cmd = [clangxx, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-attributes",
           "-Wno-ignored-attributes", f'-DGEN_SRC="{tmp_path / (name + ".hip")}"', "-DGEN_KERNELS=" + ",".join(kernels), DRIVER, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    for log_size, before, after in cases:
        path = tmp_path / f"{name}.{log_size}.bin"
        with open(path, "wb") as f:
            f.write(np.asarray([1 << log_size, log_size, len(before)], np.uint32).tobytes())
            for c in list(before) + list(after):
                f.write(np.ascontiguousarray(c, dtype=np.uint32).tobytes())
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and f"{1 << log_size} rows, 0 mismatches, 0 stored words not below p" in r.stdout, (log_size, (r.stdout + r.stderr)[-3000:])
    return len(kernels)


def _case(prog, n_cols, inputs_nat, log_size, fill=0xDEADBEEF):
    """(log_size, stored-order columns before, after): columns beyond the inputs start as `fill` (not a field element: a store that
    is missing shows)"""
    n = 1 << log_size
    nat = list(inputs_nat) + [np.full(n, fill, np.uint64) for _ in range(n_cols - len(inputs_nat))]
    want = TP.interp(prog, nat, log_size)
    return log_size, [TP.to_storage(c) for c in nat], [TP.to_storage(c) for c in want]


@pytest.mark.parametrize("vec4", ["0", "1"])
@pytest.mark.parametrize("segment", [None, "200"])
def test_opcode_table_on_the_host_under_sanitizers(nz, tmp_path, monkeypatch, segment, vec4):
    """Every new opcode on all ordered pairs of EDGE (shift counts 0, 31, 32, p-1; OR / XOR / SHL results that reach p), INV of 0, 1, p-1;
    both kernel shapes"""
    monkeypatch.setenv("NX_TRACE_VEC4", vec4)
    prog, n_cols, _ = TP.opcode_table()
    if segment:
        monkeypatch.setenv("NX_AIR_SEGMENT", segment)
    text = nz.trace_program_source(prog, n_cols)
    assert ("GW4(cols[" in text.split('extern "C"')[1]) == (vec4 == "1")
    cases = [_case(prog, n_cols, TP.opcode_table_inputs(lg), lg) for lg in (5, 7)]
    x, want = TP.opcode_table_inputs(5)[0], TP.interp(prog, TP.opcode_table_inputs(5) + [None] * (n_cols - 2), 5)
    shl_by_1 = want[2 + 12 * TP.BINARY.index("shl") + TP.EDGE.index(1)]
    assert set(int(v) for v in x[:11]) == set(TP.EDGE) and int(shl_by_1[list(x).index(1 << 30)]) == 1     # 2^31 mod p: the interpreter itself reduces
    assert int(want[-1][list(x).index(P - 1)]) == P - 1 and int(want[-1][0]) == 0                       # INV(p-1) = p-1, INV(0) = 0
    n = _run_twin(tmp_path, "table", text, cases)
    assert (n > 1) == bool(segment)


def test_offsets_and_the_row_on_the_host_under_sanitizers(nz, tmp_path):
    prog, n_cols, _ = TP.offsets_program()
    rng = np.random.default_rng(11)
    cases = [_case(prog, n_cols, [rng.integers(0, P, 1 << lg).astype(np.uint64)], lg) for lg in (5, 7)]
    a = rng.integers(0, P, 32).astype(np.uint64)
    nat = TP.interp(prog, [a] + [None] * 6, 5)
    assert "GW4(cols[" not in nz.trace_program_source(prog, n_cols).split('extern "C"')[1]      # offsets: one row per lane
    assert int(nat[1][0]) == int(a[30]) and int(nat[2][0]) == int(a[31]) and int(nat[3][31]) == int(a[0]) and int(nat[4][30]) == int(a[1])   # the wraps
    assert np.array_equal(nat[5], np.arange(32))
    _run_twin(tmp_path, "offsets", nz.trace_program_source(prog, n_cols), cases)


@pytest.mark.parametrize("vec4", ["0", "1"])
def test_store_if_on_the_host_under_sanitizers(nz, tmp_path, monkeypatch, vec4):
    monkeypatch.setenv("NX_TRACE_VEC4", vec4)
    prog, n_cols, n_in = TP.store_if_program()
    cases = []
    for lg in (5, 7):
        inputs = TP.store_if_inputs(lg)
        want = TP.interp(prog, inputs, lg)
        assert np.all(want[5][3::4] == TP.SENTINEL) and not np.any(want[5][0::4] == TP.SENTINEL)          # chip 3's rows are untouched
        cases.append((lg, [TP.to_storage(c) for c in inputs], [TP.to_storage(c) for c in want]))
    _run_twin(tmp_path, "store_if", nz.trace_program_source(prog, n_cols), cases)
