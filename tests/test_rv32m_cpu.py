"""The 32-bit integer register kind of nx_trace_program (NX_T_PACK32 .. NX_T_REMU32) and the RV32M chips recorded over it, what needs
no GPU: the opcode numbers in the four places that name them, every new refusal through the source-only form with a NULL context, the
other program kinds refusing the opcodes, the source of a program without them unchanged to the byte, the model's pins against Python's
own integers and the RISC-V rules, the recorded constraints on the model's traces (the row-wise judge of test_trace_check_cpu.py and a
proof by the CPU oracle), and the generated text of the fill program run on the host under the address and undefined-behaviour
sanitizers (tests/native/rv32m_text_host.cpp, a stand-alone program) against the model, word for word."""
import ctypes as C
import hashlib
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import rv32m_air as A
import rv32m_model as M
import trace_programs as TP
from test_air_text_host_cpu import _clangxx
from test_trace_check_cpu import interp_check
from test_trace_program_cpu import ADD, CONST, CONSTE, CONSTRAINT_B, FRACB, LOAD, NX_ERR_ARG, STORE, STORE_IF, _call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "native", "rv32m_text_host.cpp")
NAMES = ("PACK32", "LO16", "HI16", "MULLO32", "MULHU32", "DIVU32", "REMU32")
(PACK32, LO16, HI16, MULLO32, MULHU32, DIVU32, REMU32) = range(43, 50)
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    nexus_zkvm_amd.load_library()
    return nexus_zkvm_amd


# ---------------------------------------------------------------- the numbers, the header ----------
def test_opcode_numbers_agree_in_header_recorder_rust_builder_and_sys(nz):
    import nexus_zkvm_amd.air_program as ap
    header = open(nz.HEADER_PATH).read()
    sys_src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    hip = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "trace_program.rs")).read()
    for k, name in enumerate(NAMES):
        assert re.search(r"\bNX_T_%s = %d\b" % (name, 43 + k), header), name
        assert getattr(ap, "T_" + name) == 43 + k
        assert "pub const NX_T_%s: u32 = %d;" % (name, 43 + k) in sys_src, name
        assert "pub fn %s(&mut self" % name.lower() in hip and "sys::NX_T_%s," % name in hip, name
        assert callable(getattr(ap.ProgramBuilder, name.lower()))
    assert not re.search(r"\bNX_T_\w+ = (5\d|[6-9]\d)\b", header)                  # 50 and up stay unknown


def test_header_with_the_integer_opcodes_is_still_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    f = tmp_path / "h.c"
    f.write_text('#include "nexus_hip.h"\n'
                 'int g(void) { return NX_T_PACK32 + NX_T_LO16 + NX_T_HI16 + NX_T_MULLO32 + NX_T_MULHU32 + NX_T_DIVU32 + NX_T_REMU32; }\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(f), "-o", str(tmp_path / "h.o")], check=True)


# ---------------------------------------------------------------- refusals ----------
# registers 0, 1: two loaded words; 2: their PACK32, a W register
HEAD = [(LOAD, 0, 0, 0), (LOAD, 1, 0, 0), (PACK32, 2, 0, 1)]
TAIL = [(LO16, 3, 2, 0), (STORE, 0, 1, 3)]


def refusal_cases():
    """(name, instrs, n_regs, n_cols, the instruction nx_last_error must name, a word of the message) — shared with the GPU suite"""
    cases = []
    for op in (MULLO32, MULHU32, DIVU32, REMU32):
        cases.append((f"{op}: first operand is a field value", HEAD + [(op, 3, 0, 2), (LO16, 3, 3, 0), (STORE, 0, 1, 3)], 4, 2, 3, "does not hold a 32-bit integer"))
        cases.append((f"{op}: second operand is a field value", HEAD + [(op, 3, 2, 1), (LO16, 3, 3, 0), (STORE, 0, 1, 3)], 4, 2, 3, "does not hold a 32-bit integer"))
    for op in (LO16, HI16):
        cases.append((f"{op} of a field value", HEAD + [(op, 3, 1, 0), (STORE, 0, 1, 3)], 4, 2, 3, "does not hold a 32-bit integer"))
        cases.append((f"{op} with a b", HEAD + [(op, 3, 2, 1), (STORE, 0, 1, 3)], 4, 2, 3, "b of a LO16 / HI16"))
    cases += [
        ("PACK32 of a W register", HEAD + [(PACK32, 3, 2, 1)] + TAIL, 4, 2, 3, "read by a field opcode"),
        ("field sum of a W register", HEAD + [(ADD, 3, 2, 1), (STORE, 0, 1, 3)], 4, 2, 3, "read by a field opcode"),
        ("STORE of a W register", HEAD + [(STORE, 0, 1, 2)], 4, 2, 3, "read by a field opcode"),
        ("STORE_IF under a W flag", HEAD + [(STORE_IF, 2, 1, 0)], 4, 2, 3, "read by a field opcode"),
        ("STORE_IF of a W value", HEAD + [(STORE_IF, 0, 1, 2)], 4, 2, 3, "read by a field opcode"),
        # the kind is the latest writer's: register 2 is rewritten as a field value, then read as an integer
        ("a W register rewritten by a field opcode", HEAD + [(CONST, 2, 7, 0)] + TAIL, 4, 2, 4, "does not hold a 32-bit integer"),
        ("read before write", [(LOAD, 0, 0, 0), (PACK32, 2, 0, 1)] + TAIL, 4, 2, 1, "no earlier instruction wrote"),
        ("W operand never written", HEAD + [(MULLO32, 3, 2, 3)] + TAIL, 4, 2, 3, "no earlier instruction wrote"),
        ("dst out of range", HEAD + [(MULLO32, 4, 2, 2)] + TAIL, 4, 2, 3, "register out of range"),
        ("operand out of range", HEAD + [(DIVU32, 3, 2, 9)] + TAIL, 4, 2, 3, "register out of range"),
        ("opcode 50", HEAD + [(50, 3, 2, 2)] + TAIL, 4, 2, 3, "unknown opcode"),
    ]
    return cases


@pytest.mark.parametrize("case", refusal_cases(), ids=lambda c: c[0])
def test_refusals_with_a_null_context(nz, case):
    _, instrs, n_regs, n_cols, named, word = case
    rc, msg, text = _call(nz, instrs, n_regs, n_cols)
    assert rc == NX_ERR_ARG and text is None, (rc, msg)
    assert f"instruction {named}:" in msg and word in msg, msg


def test_the_smallest_valid_program_generates_and_names_its_helpers(nz):
    rc, msg, text = _call(nz, HEAD + [(DIVU32, 2, 2, 2)] + TAIL, 4, 2)
    assert rc == 0, msg
    assert "t_divu32(r2, r2)" in text and "FI u32 t_remu32(" in text and "FI u32 t_mulhu32(" in text


def test_the_other_program_kinds_refuse_the_integer_opcodes(nz):
    L = nz.load_library()
    for op in range(43, 50):
        cons = np.array([(LOAD, 0, 0, 0), (op, 1, 0, 0), (CONSTRAINT_B, 0, 0, 0)], np.uint32).reshape(-1)
        p = cons.ctypes.data_as(C.c_void_p)
        src = C.c_void_p()
        assert L.nx_air_compile(None, p, 3, 2, 2, 0, 1, None, C.byref(src)) == NX_ERR_ARG and not src.value
        assert b"malformed instruction 1" in L.nx_last_error(None)
        assert L.nx_air_check_source(p, 3, 2, 2, 0, 1, C.byref(src)) == NX_ERR_ARG and not src.value
        deg = (C.c_uint32 * 1)()
        assert L.nx_air_constraint_degrees(None, p, 3, 2, 2, 0, 1, deg) == NX_ERR_ARG
        out, n = (nz.CheckFailureC * 1)(), C.c_uint32(7)
        assert L.nx_air_check(None, p, 3, 2, (C.c_void_p * 2)(), 2, None, 0, 1, 5, out, 1, C.byref(n)) == NX_ERR_ARG and n.value == 7
        frac = np.array([(LOAD, 0, 0, 0), (CONSTE, 4, 0, 0), (op, 1, 0, 0), (FRACB, 0, 0, 4)], np.uint32).reshape(-1)
        ec = np.zeros(4, np.uint32)
        csrc = C.c_char_p()
        assert L.nx_logup_program(None, frac.ctypes.data_as(C.c_void_p), 4, 8, None, 2, ec.ctypes.data_as(C.c_void_p), 1, 5, 1, None, C.byref(csrc)) == NX_ERR_ARG
        assert b"malformed instruction 2" in L.nx_last_error(None)


# the source nx_trace_program generated for trace_programs.opcode_table() before the W kind existed (sha256; one row per lane, four)
TABLE_SOURCE_BEFORE = {"0": "b8118b53adfec463fad9558dcd2746bf43f7d187a8cca3662a783f9246c3dfc1",
                       "1": "2c2fd8a9355684ba7c8b77ea719db1648ad13720e25d1626b8b1d1088a4055af"}


@pytest.mark.parametrize("vec4", ["0", "1"])
def test_a_program_without_the_new_opcodes_generates_the_source_it_always_did(nz, monkeypatch, vec4):
    monkeypatch.setenv("NX_TRACE_VEC4", vec4)
    monkeypatch.delenv("NX_AIR_SEGMENT", raising=False)
    prog, n_cols, _ = TP.opcode_table()
    text = nz.trace_program_source(prog, n_cols)
    assert "t_divu32" not in text and "t_mulhu32" not in text
    assert hashlib.sha256(text.encode()).hexdigest() == TABLE_SOURCE_BEFORE[vec4]


# ---------------------------------------------------------------- the recorder ----------
def test_recorder_kinds_cse_and_the_operators_that_raise():
    import nexus_zkvm_amd.air_program as ap
    pb = ap.ProgramBuilder()
    (a,), (b,) = pb.next_trace_mask(0), pb.next_trace_mask(1)
    x, y = pb.pack32(a, b), pb.pack32(b, a)
    assert x.kind == "W" and pb.lo16(x).kind == "B" and pb.mullo32(x, y).kind == "W"
    assert pb.pack32(a, b).id == x.id and x.id != y.id                             # CSE; PACK32 is not commutative
    assert pb.mullo32(x, y).id == pb.mullo32(y, x).id and pb.mulhu32(x, y).id == pb.mulhu32(y, x).id
    assert pb.divu32(x, y).id != pb.divu32(y, x).id and pb.remu32(x, y).id != pb.remu32(y, x).id
    for bad in (lambda: x + a, lambda: a + x, lambda: x - 1, lambda: 1 - x, lambda: x * y, lambda: 2 * x, lambda: -x):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: pb.store(2, x), lambda: pb.store_if(x, 2, a), lambda: pb.band(x, a), lambda: pb.mullo32(a, x), lambda: pb.lo16(a), lambda: pb.pack32(x, a)):
        with pytest.raises(AssertionError):
            bad()
    pb.store(2, pb.hi16(pb.divu32(x, y)))
    prog = pb.build_trace_program()
    assert [int(i[0]) for i in prog.instrs] == [LOAD, LOAD, PACK32, PACK32, DIVU32, HI16, STORE] and prog.n_regs <= 4      # a W value takes one register


# ---------------------------------------------------------------- the model's pins ----------
def _signed(v):
    return v - (1 << 32) if v >> 31 else v


def _riscv(op, b, c):
    """The RV32M results from Python's own integers (the unprivileged specification's table for division)."""
    sb, sc = _signed(b), _signed(c)
    trunc = lambda n, d: abs(n) // abs(d) * (1 if (n < 0) == (d < 0) else -1)
    if op == "mul":
        return (b * c) & M32
    if op == "mulhu":
        return (b * c) >> 32
    if op == "mulh":
        return ((sb * sc) >> 32) & M32
    if op == "mulhsu":
        return ((sb * c) >> 32) & M32
    if op == "divu":
        return M32 if c == 0 else b // c
    if op == "remu":
        return b if c == 0 else b % c
    if op == "div":
        return M32 if c == 0 else 0x80000000 if (b, c) == (0x80000000, M32) else trunc(sb, sc) & M32
    return b if c == 0 else 0 if (b, c) == (0x80000000, M32) else (sb - trunc(sb, sc) * sc) & M32


def _word(limbs):
    return sum(int(v) << (8 * k) for k, v in enumerate(limbs))


def test_model_pins():
    rng = random.Random(7)
    pairs = M.PAIRS + [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(2000)]
    assert len(M.E) == 21 and len(M.PAIRS) == 441 and M.N_COLS == 89
    top = 0
    for b, c in pairs:
        for op in M.OPS:
            r = M.row(op, b, c)
            assert _word(r["ValueA"]) == _riscv(op, b, c), (op, hex(b), hex(c))
            assert all(0 <= v < 256 for n in M.BYTE_COLUMNS if n in r for v in r[n]) and all(v in (0, 1) for n in M.BOOL_COLUMNS if n in r for v in r[n])
            top = max(top, r["MulCarry1"][0])
            if op in ("divu", "remu", "div", "rem"):
                dividend, divisor = (b, c) if op[-1] == "u" else (abs(_signed(b)), abs(_signed(c)))
                q, t, rem, u = (_word(r[n]) for n in ("Quotient", "HelperT", "Remainder", "HelperU"))
                if divisor == 0:
                    assert (q, t, rem, u) == (M32, 0, dividend, 0) and r["IsDivideByZero"] == [1] and r["HelperUBorrow"] == [0]
                else:
                    assert (q, rem) == divmod(dividend, divisor) and t == q * divisor and u == divisor - rem - 1 and r["IsDivideByZero"] == [0]
            if op in ("mulh", "mulhsu"):
                assert (_word(r["ValueAAbsHigh"]) << 32) | _word(r["ValueAAbs"]) == abs(_signed(b) * (_signed(c) if op == "mulh" else c))
                assert _word(r["ValueALow"]) == (b * c) & M32
    assert 3 <= top <= 4 and M.mull(0x1AEA93FB, 0xC0E3CAF2)["carry"][1] == 4             # MulCarry1 reaches 4 (rarely): range8, not a boolean
    # the quirks by name
    r = M.row("div", 0x80000000, M32)
    assert r["IsOverflow"] == [1] and _word(r["Quotient"]) == 0x80000000 and _word(r["Remainder"]) == 0 and r["ValueAAbsBorrow"] == [0, 0] and r["SgnA"] == [1]
    assert M.row("rem", 0x80000000, M32)["IsOverflow"] == [1] and M.row("div", 0x80000000, 1)["IsOverflow"] == [0]
    # which of quotient / remainder feeds ValueAAbsBorrow (a carry at bit 16 of ~v + 1 needs a negative v whose low half is 0):
    # -0x30000 / 0x10000 = -3 rem 0: neither; a zero divisor: REM keeps the dividend -0x10000, DIV's -1 has no carries by decree;
    # -0x10000 / 1 = -0x10000 rem 0: the quotient only
    assert M.row("div", 0xFFFD0000, 0x10000)["ValueAAbsBorrow"] == [0, 0] and M.row("rem", 0xFFFD0000, 0x10000)["ValueAAbsBorrow"] == [0, 0]
    assert M.row("rem", 0xFFFF0000, 0)["ValueAAbsBorrow"] == [1, 0] and M.row("div", 0xFFFF0000, 0)["ValueAAbsBorrow"] == [0, 0]
    assert M.row("div", 0xFFFF0000, 1)["ValueAAbsBorrow"] == [1, 0] and M.row("rem", 0xFFFF0000, 1)["ValueAAbsBorrow"] == [0, 0]
    # a chip writes its own columns only
    assert "MulP5" not in M.row("mul", 3, 5) and "MulP1" not in M.row("mulhu", 3, 5) and "SgnC" not in M.row("mulhsu", M32, M32)
    # rows without an M flag: the M columns are 0, ValueA keeps what it held
    ops, operands = M.trace_ops("div")
    before, after = M.seeds_and_trace(ops, operands)
    idle = np.array([o is None for o in ops])
    assert idle.sum() == 71 and all(np.all(after[k][idle] == (M.SENTINEL if k in M.cols_of("ValueA") else 0)) for k in range(M.N_SEED, M.N_COLS))
    assert not np.any(after[M.COL["ValueA"]][~idle] == M.SENTINEL)


def test_interpreter_of_the_integer_opcodes_on_the_pairs():
    prog = A.opcode_table()
    ins = A.opcode_table_inputs(9)
    out = M.interp(prog, ins + [None] * (A.TABLE_COLS - A.TABLE_INPUTS), 9)
    word = lambda k, i: int(out[k][i]) | (int(out[k + 1][i]) << 16)
    for i, (x, y) in enumerate(M.PAIRS):
        assert word(4, i) == x
        assert (word(8, i), word(10, i)) == ((x * y) & M32, (x * y) >> 32)
        assert (word(12, i), word(14, i)) == ((M32, x) if y == 0 else divmod(x, y))
    lo, hi = int(ins[0][20]) * 0x7FFF + int(ins[3][20]), int(ins[1][20]) * 3 + int(ins[2][20]) * 0x10001
    assert hi >= 1 << 16 and word(6, 20) == (lo % TP.P + ((hi % TP.P) << 16)) & M32             # PACK32 truncates


# ---------------------------------------------------------------- the constraints ----------
@pytest.fixture(scope="module")
def component():
    comp = A.constraints(M.LOG, tree=0)
    comp.log_constraint_degree_bound = 2           # the v1 main component's: a DIV selector times a sign select is degree 4
    return comp


@pytest.mark.parametrize("op", M.OPS)
def test_recorded_constraints_hold_on_every_row(oracle, component, op):
    ops, operands = M.trace_ops(op)
    _, trace = M.seeds_and_trace(ops, operands, sentinel=0xA5)
    assert interp_check(component.program, trace, M.LOG) == {}
    ocfg = O.default_cfg(pow_bits=2, log_constraint_degree=2)
    s = O.ProverSession(ocfg, M.LOG)
    root = s.commit([TP.to_storage(c).astype(np.uint32) for c in trace])
    words = s.prove([component])
    v = O.VerifierSession(ocfg)
    v.commit(root, [M.LOG] * M.N_COLS)
    assert v.verify([component], words) is None


@pytest.mark.parametrize("op", ["divu", "remu"])
def test_one_changed_quotient_byte_fails_divu_remu_constraints_on_its_row_only(component, op):
    ops, operands = M.trace_ops(op)
    _, trace = M.seeds_and_trace(ops, operands, sentinel=0xA5)
    row = M.PAIRS.index((0xAAAAAAAB, 3))
    trace[M.COL["Quotient"] + 1][row] ^= 1
    bad = interp_check(component.program, trace, M.LOG)
    assert bad and all(component.chips[j] == "DivuRemu" and n_rows == 1 and first == row for j, (n_rows, first, _) in bad.items()), bad


def test_every_chip_has_its_constraints(component):
    assert component.program.n_constraints == len(component.chips) == 112
    assert set(component.chips) == {"Mul", "Mulhu", "MulhMulhsu", "DivuRemu", "DivRem", "bool"}


# ---------------------------------------------------------------- the generated text on the host ----------
def _build_twin(tmp_path, name, text):
    (tmp_path / f"{name}.hip").write_text(text)
    kernels = re.findall(r'extern "C" __attribute__\(\(global\)\)[^\n]*? void (\w+)\(', text)
    assert kernels and kernels[0] == "air_kernel"
    exe = str(tmp_path / name)
    cmd = [_clangxx(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-attributes",
           "-Wno-ignored-attributes", f'-DGEN_SRC="{tmp_path / (name + ".hip")}"', "-DGEN_KERNELS=" + ",".join(kernels), DRIVER, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    return exe, len(kernels)


def _operand_file(path, log_size, before, after):
    with open(path, "wb") as f:
        f.write(np.asarray([log_size, len(before)], np.uint32).tobytes())
        for c in list(before) + list(after):
            f.write(np.ascontiguousarray(TP.to_storage(c), dtype=np.uint32).tobytes())
    return str(path)


def _source(nz, prog, n_cols, log_size):
    """the text the library runs at this log size: two rows never take the four-positions-per-lane kernel"""
    rc, msg, text = _call(nz, prog.instrs, prog.n_regs, n_cols, None, log_size)
    assert rc == 0, msg
    return text


def _run_on_host(nz, tmp_path, prog, n_cols, cases, vec4):
    """cases: (log_size, natural columns before, natural columns after).  One twin per distinct text; returns the texts by log size."""
    texts, by_text = {}, {}
    for log_size, before, after in cases:
        texts[log_size] = _source(nz, prog, n_cols, log_size)
        assert ("GW4(cols[" in texts[log_size].split('extern "C"')[1]) == (vec4 == "1" and log_size >= 2)
        by_text.setdefault(texts[log_size], []).append(_operand_file(tmp_path / f"case{len(texts)}_{len(by_text)}.{log_size}.bin", log_size, before, after))
    for k, (text, files) in enumerate(by_text.items()):
        exe, _ = _build_twin(tmp_path, f"twin{k}", text)
        r = subprocess.run([exe] + files, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.count(" rows, 0 mismatches") == len(files), (r.stdout + r.stderr)[-3000:]
    return texts


@pytest.mark.parametrize("vec4", ["0", "1"])
@pytest.mark.parametrize("segment", [None, "200"])
def test_fill_program_text_on_the_host_under_sanitizers_equals_the_model(nz, tmp_path, monkeypatch, segment, vec4):
    """log sizes 1 (two rows: never four per lane), 2 and 9, each of the eight opcodes; "air.segment" at its smallest cuts after every
    store, so the four Quotient bytes, fed by one division, fall into different kernels and each recomputes it"""
    monkeypatch.setenv("NX_TRACE_VEC4", vec4)
    if segment:
        monkeypatch.setenv("NX_AIR_SEGMENT", segment)
    prog = A.fill_program()
    cases = []
    for log_size in (1, 2, 9):
        for op in M.OPS:
            ops, operands = M.trace_ops(op, log_size)
            cases.append((log_size,) + M.seeds_and_trace(ops, operands))
    texts = _run_on_host(nz, tmp_path, prog, M.N_COLS, cases, vec4)
    kernels = texts[9].split('extern "C"')[1:]
    if segment:
        stores = lambda kernel, col: re.search(r"(\bo%d\[0\]|GW\(cols\[%d\]\)\[r\]) = " % (col, col), kernel)
        quotient = [k for k in kernels if any(stores(k, col) for col in M.cols_of("Quotient"))]
        assert len(kernels) > 20 and len(quotient) >= 2 and all("t_divu32(" in k for k in quotient)
    else:
        assert len(kernels) <= 2                 # the default budget: one kernel with a row per lane, two with four positions per lane


@pytest.mark.parametrize("vec4", ["0", "1"])
def test_opcode_table_text_on_the_host_under_sanitizers(nz, tmp_path, monkeypatch, vec4):
    monkeypatch.setenv("NX_TRACE_VEC4", vec4)
    prog = A.opcode_table()
    cases = []
    for log_size in (1, 2, 6, 9):
        before = A.opcode_table_inputs(log_size) + [np.full(1 << log_size, 0xDEADBEEF, np.uint64)] * (A.TABLE_COLS - A.TABLE_INPUTS)
        cases.append((log_size, before, M.interp(prog, before, log_size)))
    _run_on_host(nz, tmp_path, prog, A.TABLE_COLS, cases, vec4)


def test_fill_program_compiles_for_gfx950(nz, tmp_path, monkeypatch):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    for vec4 in "01":
        monkeypatch.setenv("NX_TRACE_VEC4", vec4)
        f = tmp_path / f"fill{vec4}.hip"
        f.write_text(nz.trace_program_source(A.fill_program(), M.N_COLS))
        subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-c", str(f), "-o", str(tmp_path / f"fill{vec4}.o")], check=True, timeout=300)
