"""nx_trace_keccak_memory_check, what needs no GPU: the export and its mirrors, every refusal with a NULL context, the model against
hashlib, PermutationMemoryCheckEval restated (tests/keccak_memcheck_air.py) over the model's columns on the CPU oracle — every row
of every shape, the one failing constraint of the shapes that wrap, the balance of the closed statement — and the column emitter of
csrc/keccak_memcheck.h, the text the kernel compiles, built as a stand-alone host program under ASan + UBSan
(tests/native/keccak_memcheck_host.cpp) and compared word for word with the model."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import keccak_memcheck_model as MM
import keccak_round_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX_ERR_ARG = -2
SHAPE_IDS = [MM.shape_id(s) for s in MM.SHAPES]


def _lib():
    import nexus_zkvm_amd as nz
    if not os.path.exists(nz.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nz, nz.load_library()


def test_symbol_is_declared_exported_and_mirrored():
    nz, lib = _lib()
    assert "nx_trace_keccak_memory_check" in nz.declared_symbols()
    assert hasattr(lib, "nx_trace_keccak_memory_check")
    assert hasattr(nz.HipBackend, "trace_keccak_memory_check")
    header = open(nz.HEADER_PATH).read()
    assert re.search(r"#define NX_KECCAK_MEMCHECK_MAIN_COLS\s+%d\b" % MM.MAIN_COLS, header) and re.search(r"#define NX_KECCAK_MEMCHECK_PRE_COLS\s+%d\b" % MM.PRE_COLS, header)
    assert "MODULO 2^32" in header[header.index("PermutationMemoryCheck"):header.index("int nx_trace_keccak_memory_check")]
    assert (nz.KECCAK_MEMCHECK_MAIN_COLS, nz.KECCAK_MEMCHECK_PRE_COLS) == (MM.MAIN_COLS, MM.PRE_COLS)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sys_src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    assert "pub fn nx_trace_keccak_memory_check(ctx: *mut nx_ctx, d_states: *const u64, d_addresses: *const u32, d_timestamps: *const u32, n_instances: u32, " \
           "log_size: u32, d_main: *const *mut u32, d_pre: *const *mut u32, d_states_out: *mut u64) -> c_int;" in sys_src
    hip = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "lib.rs")).read()
    assert "pub unsafe fn trace_keccak_memory_check(&mut self" in hip and "sys::nx_trace_keccak_memory_check(" in hip
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "nx_trace_keccak_memory_check" in open(os.path.join(ROOT, doc)).read(), doc


class _Call:
    """A well-formed call made of host-only numbers that are never followed (the context is NULL), one piece of which a test breaks."""

    def __init__(self, lib):
        self.lib, self.f = lib, lib.nx_trace_keccak_memory_check
        self.f.restype = C.c_int
        self.f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.main = (C.c_void_p * MM.MAIN_COLS)(*[0x100000 + 0x1000 * k for k in range(MM.MAIN_COLS)])
        self.pre = (C.c_void_p * MM.PRE_COLS)(0x4000000)
        self.a = dict(states=0x8000000, addresses=0xA000000, timestamps=0xB000000, n=3, log_size=2, main=True, pre=True, out=0x9000000)

    def __call__(self, **kw):
        a = dict(self.a, **kw)
        rc = self.f(None, a["states"], a["addresses"], a["timestamps"], a["n"], a["log_size"], C.addressof(self.main) if a["main"] else None,
                    C.addressof(self.pre) if a["pre"] else None, a["out"])
        return rc, self.lib.nx_last_error(None).decode()


def test_every_refusal_is_reached_with_a_null_context_and_names_its_argument():
    nz, lib = _lib()

    def refused(text, build=lambda c: None, **kw):
        c = _Call(lib)
        build(c)
        rc, msg = c(**kw)
        assert rc == NX_ERR_ARG and msg.startswith("nx_trace_keccak_memory_check: ") and text in msg, (rc, msg, text)

    refused("NULL context")                                          # everything else well formed
    refused("log_size of 0", log_size=0, n=0)
    refused("log_size of 31", log_size=31)
    refused("n_instances of 5", n=5)                                 # 5 rows in 2^2
    refused("n_instances of 4294967295", n=0xFFFFFFFF, log_size=30)
    refused("NULL d_main", main=False)
    refused("d_main[1234] is NULL", lambda c: c.main.__setitem__(1234, None))
    refused("d_pre[0] is NULL", lambda c: c.pre.__setitem__(0, None))
    refused("d_main[2000] has the pointer of d_main[7]", lambda c: c.main.__setitem__(2000, c.main[7]))
    refused("d_pre[0] has the pointer of d_main[200]", lambda c: c.pre.__setitem__(0, c.main[200]))
    refused("NULL d_states", states=None)
    refused("NULL d_addresses", addresses=None)
    refused("NULL d_timestamps", timestamps=None)
    refused("d_states is not 8-byte aligned", states=0x8000004)
    refused("d_states_out is not 8-byte aligned", out=0x9000004)
    refused("d_timestamps is not 16-byte aligned", timestamps=0xB000008)
    refused("d_timestamps is not 16-byte aligned", timestamps=0xB000004)
    refused("d_states_out overlaps d_states", out=0x8000000)
    refused("d_states_out overlaps d_states", out=0x8000000 + 3 * 200 - 8)
    refused("d_states_out overlaps d_states", out=0x8000000 - 3 * 200 + 8)
    # not refused for their own sake: no instances and no inputs, no preprocessed column, no output states, output right behind the
    # input, a full trace — the NULL context is all that is left to object to
    refused("NULL context", states=None, addresses=None, timestamps=None, n=0)
    refused("NULL context", pre=False, out=None)
    refused("NULL context", out=0x8000000 + 3 * 200)
    refused("NULL context", n=4)
    refused("NULL context", n=1 << 30, log_size=30, out=None)


# ------------------------------------------------------------------------------------------------------------------- the model ----
def test_model_out_state_of_a_padded_block_is_sha3_256():
    msgs = [b"", b"abc", bytes(range(135))]
    states = np.stack([M.sha3_256_block(m) for m in msgs])
    w = MM.fill(states, [0, 1, 2], np.zeros((3, 200), np.uint32), 2, natural=True)
    for r, m in enumerate(msgs):
        assert bytes(w["main"][MM.OUT:MM.OUT + 32, r].astype(np.uint8)) == hashlib.sha3_256(m).digest()
        assert M.digest(w["out"][r]) == hashlib.sha3_256(m).digest()
        assert bytes(w["main"][MM.IN:MM.IN + 200, r].astype(np.uint8)) == np.asarray(states[r], "<u8").tobytes()


def test_model_column_order_is_the_stated_layout():
    """the reference's own prove_keccak input: address 0xFFFE and every timestamp 0xFFFE; a carry at byte 1; padding rows 0 but is_padding"""
    states, addresses, ts = MM.inputs(4)
    assert (addresses == 0xFFFE).all() and (ts == 0xFFFE).all()
    m = MM.fill(states, addresses, ts, 4, natural=True)
    main, pre = m["main"], m["pre"]
    assert main.shape == (2001, 16) and pre.shape == (1, 16)
    col = lambda k: main[k, 3]
    assert (col(MM.ADDR), col(MM.ADDR + 1), col(MM.ADDR + 2), col(MM.ADDR + 3), col(MM.ADDR + 4), col(MM.ADDR + 5)) == (0xFFFE, 0, 0xFFFF, 0, 0, 1)
    assert main[MM.ADDR_CARRY:MM.ADDR_CARRY + 200, 3].tolist() == [0, 1] + [0] * 198
    assert main[MM.PREV_TS:MM.PREV_TS + 400, 3].tolist() == [0xFFFE, 0] * 200 and main[MM.NEXT_TS:MM.NEXT_TS + 400, 3].tolist() == [0xFFFF, 0] * 200
    assert not main[MM.TS_CARRY:MM.TS_CARRY + 200, 3].any()
    assert main[MM.IN + 8 * 7 + 2, 3] == (int(states[3][7]) >> 16) & 255
    assert main[MM.IS_PADDING].tolist() == [0] * 15 + [1] and not main[:MM.IS_PADDING, 15].any()          # out_state of a padding row is 0 too
    assert pre[0].tolist() == [0] * 15 + [1]
    # 0xFF38 + 199 = 0xFFFF: the last carry is flagged; a timestamp of 0xFFFF carries into the high limb
    states, addresses, ts = MM.inputs(2)
    main = MM.fill(states, addresses, ts, 1, natural=True)["main"]
    assert main[MM.ADDR_CARRY:MM.ADDR_CARRY + 200, 0].tolist() == [0] * 199 + [1] and main[MM.ADDR + 399, 0] == 0
    assert main[MM.TS_CARRY:MM.TS_CARRY + 200, 0].all() and main[MM.NEXT_TS:MM.NEXT_TS + 400, 0].tolist() == [0, 1] * 200
    assert np.array_equal(MM.want(2)["main"], M.to_storage(main, 1))


# --------------------------------------------------------------------------------------------------------------- the constraints ----
@pytest.fixture(scope="module")
def recorded():
    """memcheck_program recorded once with drawn elements -> (the builder, the constraint program, its column count)"""
    import nexus_zkvm_amd.air_program as ap
    import keccak_memcheck_air as A
    drawn = np.random.default_rng(69).integers(1, M.P, size=(10, 4), dtype=np.uint32)
    elems = {name: (drawn[2 * k], drawn[2 * k + 1]) for k, (name, _) in enumerate(A.RELATIONS)}
    pb = A.memcheck_program(ap, elems, (0, 0, 0, 0))
    return pb, pb.build(), A.MAIN + A.PRE + 4 * A.LOGUP_COLS, elems


def test_recorded_program_has_the_counts_of_the_component(recorded):
    pb, prog, n_cols, _ = recorded
    frac = pb.build_logup()
    assert (prog.n_constraints, frac.n_logup_cols, len(pb.fractions)) == (802, 201, 402)
    assert sorted(prog.masks) == list(range(n_cols)) and n_cols == 2806
    assert prog.masks[MM.IS_PADDING] == [0, 1] and prog.masks[MM.MAIN_COLS] == [0]
    assert all(prog.masks[k] == [0] for k in range(MM.IS_PADDING))
    assert all(prog.masks[k] == ([0] if k < n_cols - 4 else [-1, 0]) for k in range(MM.MAIN_COLS + 1, n_cols))
    assert (len(prog.instrs), len(frac.instrs)) == (PROGRAM_INSTRS, FRACTION_INSTRS)


PROGRAM_INSTRS, FRACTION_INSTRS = 11125, 6412          # the recorded constraint and fraction programs, as the AIR file's docstring states them


def _plain(recorded, k, weights):
    """the sum of weights[j] x plain constraint j on every natural row of shape k's model columns (the logup constraints weigh 0: the
    interaction columns are not part of this check) -> (2^log_size, 4)"""
    import oracle_lib as O
    pb, prog, n_cols, _ = recorded
    log_size = MM.SHAPES[k][0]
    w = MM.want(k)
    zero = np.zeros(1 << log_size, np.uint32)
    cols = list(w["main"]) + list(w["pre"]) + [zero] * (n_cols - MM.MAIN_COLS - MM.PRE_COLS)
    pw = np.zeros((prog.n_constraints, 4), np.uint32)
    pw[:MM.PLAIN_CONSTRAINTS] = weights
    acc = O.eval_constraint_program(prog, cols, pw, np.ones(1, np.uint32), log_size, log_size)
    nat = np.stack(acc, axis=1)[M.pos_of_coset_row(np.arange(1 << log_size), log_size)]
    return nat


@pytest.mark.parametrize("k", range(len(MM.SHAPES)), ids=SHAPE_IDS)
def test_recorded_constraints_hold_on_every_row_of_the_models_columns(recorded, k):
    """On a shape without a wrapping value every plain constraint is 0 on every row.  On a wrapping shape exactly the expected
    constraint fails and exactly on the expected row: the random combination of all constraints is not 0 there and 0 on every other
    row, the expected constraint alone is not 0 there, and the combination without it is 0 everywhere."""
    weights = np.random.default_rng(70 + k).integers(1, M.P, size=(MM.PLAIN_CONSTRAINTS, 4), dtype=np.uint32)
    failing = np.flatnonzero(_plain(recorded, k, weights).any(axis=1)).tolist()
    if k not in MM.WRAPPING:
        assert failing == []
        return
    ordinal, row = MM.WRAPPING[k]
    assert failing == [row]
    alone = np.zeros_like(weights)
    alone[ordinal] = (1, 0, 0, 0)
    got = _plain(recorded, k, alone)
    assert np.flatnonzero(got.any(axis=1)).tolist() == [row]
    assert got[row].tolist() == [(-(1 << 16)) % M.P, 0, 0, 0]          # next high limb 0 - previous high limb 0xFFFF - carry 1
    weights[ordinal] = 0
    assert not _plain(recorded, k, weights).any()


def test_closed_statement_balances_on_the_cpu_oracle_over_the_models_columns():
    """The statement of tests/test_gpu_keccak_memcheck.py without a GPU, by the method of test_keccak_round_cpu.py: the seven claimed
    sums from the CPU oracle's logup_program over the models' columns cancel, none is zero, and one changed out_state byte of
    mem_check breaks the balance."""
    import oracle_lib as O
    import nexus_zkvm_amd.air_program as ap
    import keccak_memcheck_air as A
    states, addresses, timestamps = A.statement_inputs()
    drawn = np.random.default_rng(69).integers(1, M.P, size=(10, 4), dtype=np.uint32)
    elems = {name: (drawn[2 * k], drawn[2 * k + 1]) for k, (name, _) in enumerate(A.RELATIONS)}
    fracs = {name: p.build_logup() for name, p in A.statement_programs(ap, elems, {n: (0, 0, 0, 0) for n in A.COMPONENTS}).items()}
    assert fracs["mem_check"].n_logup_cols == MM.LOGUP_COLS and fracs["mem_side"].n_logup_cols == 1

    def claimed(pre, main, only=A.COMPONENTS, base=None):
        out = dict(base or {})
        for name in only:
            pc, mc = pre[A.PRE_AT.get(name, 0):A.PRE_AT.get(name, 0) + A.N_PRE[name]], main[A.MAIN_AT[name]:A.MAIN_AT[name] + A.N_MAIN[name]]
            cols = (pc + mc) if name in A.KEY_BITS else (mc + pc)        # a table program reads its tuple first
            inter = O.logup_program(fracs[name], cols + [None] * A.N_INT[name], A.COMP_LOG[name], fracs[name].n_logup_cols)
            out[name] = O.logup_finalize_last(inter[-1])[1]
        return out

    pre, main, final = A.host_statement(states, addresses, timestamps)
    assert np.array_equal(final, MM.keccak_f(states))
    ok = claimed(pre, main)
    assert A.total(ok) == [0, 0, 0, 0] and all(ok[name].any() for name in A.COMPONENTS)
    k = A.MAIN_AT["mem_check"] + MM.OUT + 17
    main[k] = main[k].copy()
    main[k][int(M.pos_of_coset_row(1, A.LOG_MC))] ^= 1
    assert A.total(claimed(pre, main, only=("mem_check",), base=ok)) != [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------- the shared header on the host ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/native/keccak_memcheck_host.cpp with its own main, built with the sanitizers; nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("keccak_memcheck_host")
    exe = str(d / "keccak_memcheck_host")
    subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas",
                    "-I" + os.path.join(ROOT, "nexus-zkvm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "keccak_memcheck_host.cpp"), "-o", exe], check=True, capture_output=True)
    return d, exe


@pytest.mark.parametrize("k", range(len(MM.SHAPES)), ids=SHAPE_IDS)
def test_shared_header_fills_the_models_columns_on_the_host_under_sanitizers(host_program, k):
    d, exe = host_program
    log_size, n_inst = MM.SHAPES[k][:2]
    states, addresses, ts = MM.inputs(k)
    want = MM.want(k)
    fin, fout = str(d / ("in_%d.bin" % k)), str(d / ("out_%d.bin" % k))
    with open(fin, "wb") as f:
        f.write(states.astype("<u8").tobytes() + addresses.astype("<u4").tobytes() + ts.astype("<u4").tobytes())
    r = subprocess.run([exe, str(n_inst), str(log_size), fin, fout], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    n = 1 << log_size
    raw = np.fromfile(fout, np.uint32)
    assert len(raw) == (MM.MAIN_COLS + MM.PRE_COLS) * n + 50 * n_inst
    main, pre = raw[:MM.MAIN_COLS * n].reshape(MM.MAIN_COLS, n), raw[MM.MAIN_COLS * n:(MM.MAIN_COLS + MM.PRE_COLS) * n].reshape(MM.PRE_COLS, n)
    out = raw[(MM.MAIN_COLS + MM.PRE_COLS) * n:].view("<u8").reshape(n_inst, 25)
    for c in np.flatnonzero((main != want["main"]).any(axis=1))[:1]:
        raise AssertionError("main column %d differs at positions %s" % (c, np.flatnonzero(main[c] != want["main"][c])[:8]))
    assert np.array_equal(pre, want["pre"]) and np.array_equal(out, want["out"])
