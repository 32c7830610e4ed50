"""nx_trace_keccak_round, what needs no GPU: the export and its mirrors, every refusal with a NULL context, and the round and column
emitter of csrc/keccak_round.h — the text the kernel compiles — built as a stand-alone host program under ASan + UBSan
(tests/native/keccak_round_host.cpp) and compared word for word with the model of tests/keccak_round_model.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import keccak_round_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX_ERR_ARG = -2


def _lib():
    import nexus_zkvm_amd as nz
    if not os.path.exists(nz.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nz, nz.load_library()


def test_symbol_is_declared_exported_and_mirrored():
    nz, lib = _lib()
    assert "nx_trace_keccak_round" in nz.declared_symbols()
    assert hasattr(lib, "nx_trace_keccak_round")
    assert hasattr(nz.HipBackend, "trace_keccak_round")
    header = open(nz.HEADER_PATH).read()
    assert re.search(r"#define NX_KECCAK_ROUND_MAIN_COLS\s+%d\b" % M.MAIN_COLS, header) and re.search(r"#define NX_KECCAK_ROUND_PRE_COLS\s+%d\b" % M.PRE_COLS, header)
    assert (nz.KECCAK_ROUND_MAIN_COLS, nz.KECCAK_ROUND_PRE_COLS) == (M.MAIN_COLS, M.PRE_COLS)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sys_src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    assert "pub fn nx_trace_keccak_round(ctx: *mut nx_ctx, d_states: *const u64, n_instances: u32, first_round: u32, log_rounds: u32, log_size: u32, " \
           "d_main: *const *mut u32, d_pre: *const *mut u32, d_states_out: *mut u64) -> c_int;" in sys_src
    hip = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "lib.rs")).read()
    assert "pub unsafe fn trace_keccak_round(&mut self" in hip and "sys::nx_trace_keccak_round(" in hip


class _Call:
    """A well-formed call made of host-only numbers that are never followed (the context is NULL), one piece of which a test breaks."""

    def __init__(self, lib):
        self.lib, self.f = lib, lib.nx_trace_keccak_round
        self.f.restype = C.c_int
        self.f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.main = (C.c_void_p * M.MAIN_COLS)(*[0x100000 + 0x1000 * k for k in range(M.MAIN_COLS)])
        self.pre = (C.c_void_p * M.PRE_COLS)(*[0x4000000 + 0x1000 * k for k in range(M.PRE_COLS)])
        self.a = dict(states=0x8000000, n=3, first=0, log_rounds=4, log_size=6, main=True, pre=True, out=0x9000000)

    def __call__(self, **kw):
        a = dict(self.a, **kw)
        rc = self.f(None, a["states"], a["n"], a["first"], a["log_rounds"], a["log_size"], C.addressof(self.main) if a["main"] else None,
                    C.addressof(self.pre) if a["pre"] else None, a["out"])
        return rc, self.lib.nx_last_error(None).decode()


def test_every_refusal_is_reached_with_a_null_context_and_names_its_argument():
    nz, lib = _lib()

    def refused(text, build=lambda c: None, **kw):
        c = _Call(lib)
        build(c)
        rc, msg = c(**kw)
        assert rc == NX_ERR_ARG and msg.startswith("nx_trace_keccak_round: ") and text in msg, (rc, msg, text)

    refused("NULL context")                                          # everything else well formed
    refused("first_round of 16 and log_rounds of 4", first=16)       # 16 + 16 > 24
    refused("first_round of 24 and log_rounds of 0", first=24, log_rounds=0)
    refused("first_round of 0 and log_rounds of 5", log_rounds=5)
    refused("first_round of 4294967295", first=0xFFFFFFFF, log_rounds=0)
    refused("log_rounds of 32", log_rounds=32)
    refused("log_size of 0", log_size=0, n=0)
    refused("log_size of 31", log_size=31)
    refused("n_instances of 5", n=5)                                 # 80 rows in 2^6
    refused("n_instances of 4294967295", n=0xFFFFFFFF, log_size=30)
    refused("NULL d_main", main=False)
    refused("d_main[1234] is NULL", lambda c: c.main.__setitem__(1234, None))
    refused("d_pre[8] is NULL", lambda c: c.pre.__setitem__(8, None))
    refused("d_main[1704] has the pointer of d_main[7]", lambda c: c.main.__setitem__(1704, c.main[7]))
    refused("d_pre[3] has the pointer of d_pre[0]", lambda c: c.pre.__setitem__(3, c.pre[0]))
    refused("d_pre[2] has the pointer of d_main[200]", lambda c: c.pre.__setitem__(2, c.main[200]))
    refused("NULL d_states", states=None)
    refused("d_states is not 8-byte aligned", states=0x8000004)
    refused("d_states_out overlaps d_states", out=0x8000000)
    refused("d_states_out overlaps d_states", out=0x8000000 + 3 * 200 - 8)
    refused("d_states_out overlaps d_states", out=0x8000000 - 3 * 200 + 8)
    # not refused for their own sake: no instances and no states, no preprocessed columns, no output states, output right behind the
    # input, a full trace — the NULL context is all that is left to object to
    refused("NULL context", states=None, n=0)
    refused("NULL context", pre=False, out=None)
    refused("NULL context", out=0x8000000 + 3 * 200)
    refused("NULL context", n=4)
    refused("NULL context", first=16, log_rounds=3)
    refused("NULL context", first=23, log_rounds=0, n=64)


def test_tables_of_the_header_are_fips_202s():
    """RC and the rotation offsets are literals in csrc/keccak_round.h; the model derives them (LFSR, the (t + 1)(t + 2) / 2 walk) and is
    pinned to hashlib on import."""
    text = open(os.path.join(ROOT, "nexus-zkvm_amd", "csrc", "keccak_round.h")).read()
    rc = [int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]{16})ull", text[text.index("NX_HD u64 kr_rc"):text.index("return rc[round]")])]
    assert rc == M.RC
    rot = re.search(r"constexpr u32 rot\[KR_LANES\] = \{([^}]*)\}", text).group(1)
    assert [int(x) for x in rot.split(",")] == M.ROT


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/native/keccak_round_host.cpp with its own main, built with the sanitizers; nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("keccak_round_host")
    exe = str(d / "keccak_round_host")
    subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas",
                    "-I" + os.path.join(ROOT, "nexus-zkvm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "keccak_round_host.cpp"), "-o", exe], check=True, capture_output=True)
    return d, exe


@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_shared_header_fills_the_models_columns_on_the_host_under_sanitizers(host_program, shape):
    d, exe = host_program
    n_inst, first, log_rounds, log_size = shape
    states = M.test_states(n_inst, seed=log_size)
    want = M.fill(states, first, log_rounds, log_size)
    fin, fout = str(d / ("in_%d_%d.bin" % (n_inst, first))), str(d / ("out_%d_%d.bin" % (n_inst, first)))
    states.astype("<u8").tofile(fin)
    r = subprocess.run([exe] + [str(x) for x in shape] + [fin, fout], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
    n = 1 << log_size
    raw = np.fromfile(fout, np.uint32)
    assert len(raw) == (M.MAIN_COLS + M.PRE_COLS) * n + 50 * n_inst
    main, pre = raw[:M.MAIN_COLS * n].reshape(M.MAIN_COLS, n), raw[M.MAIN_COLS * n:(M.MAIN_COLS + M.PRE_COLS) * n].reshape(M.PRE_COLS, n)
    out = raw[(M.MAIN_COLS + M.PRE_COLS) * n:].view("<u8").reshape(n_inst, 25)
    for k in np.flatnonzero((main != want["main"]).any(axis=1))[:1]:
        raise AssertionError("main column %d differs at positions %s" % (k, np.flatnonzero(main[k] != want["main"][k])[:8]))
    assert np.array_equal(pre, want["pre"]) and np.array_equal(out, want["out"])


def test_model_padding_rows_are_the_round_of_the_zero_state():
    """a padding row: zero inputs, the iota output is the round-constant bytes, everything else 0, is_padding 1"""
    w = M.fill(M.test_states(1), 16, 3, 4, natural=True)
    main, pre = w["main"], w["pre"]
    assert main[-1].tolist() == [0] * 8 + [1] * 8 and pre[8].tolist() == [0] * 15 + [1]
    for r in range(8, 16):
        rc = [(M.RC[16 + r % 8] >> (8 * b)) & 255 for b in range(8)]
        assert pre[:8, r].tolist() == rc and main[1696:1704, r].tolist() == rc and not main[:1696, r].any()
    assert pre[:8, 3].tolist() == [(M.RC[19] >> (8 * b)) & 255 for b in range(8)]


def test_restated_statement_balances_on_the_cpu_oracle_over_the_models_columns():
    """The statement of tests/test_gpu_keccak_round.py without a GPU: KeccakRoundEval restated (tests/keccak_air.py) over the model's
    columns, the tables' multiplicities counted with numpy, the interaction traces from the CPU oracle's logup_program — the seven
    claimed sums cancel, none is zero, and one changed xor output byte breaks the balance."""
    import oracle_lib as O
    import nexus_zkvm_amd.air_program as ap
    import keccak_air as K
    states = M.test_states(K.N_INST, seed=7)
    drawn = np.random.default_rng(68).integers(1, M.P, size=(8, 4), dtype=np.uint32)
    elems = {name: (drawn[2 * k], drawn[2 * k + 1]) for k, (name, _) in enumerate(K.RELATIONS)}
    fracs = {name: p.build_logup() for name, p in K.statement_programs(ap, elems, {n: (0, 0, 0, 0) for n in K.COMPONENTS}).items()}
    assert fracs["round_a"].n_logup_cols == M.LOGUP_COLS and np.array_equal(fracs["round_a"].instrs, fracs["round_b"].instrs)

    def claimed(pre, main):
        out = {}
        for name in K.COMPONENTS:
            pc, mc = pre[K.PRE_AT.get(name, 0):K.PRE_AT.get(name, 0) + K.N_PRE[name]], main[K.MAIN_AT[name]:K.MAIN_AT[name] + K.N_MAIN[name]]
            cols = (pc + mc) if name in K.KEY_BITS else (mc + pc)        # a table program reads its tuple first
            inter = O.logup_program(fracs[name], cols + [None] * K.N_INT[name], K.COMP_LOG[name], fracs[name].n_logup_cols)
            out[name] = O.logup_finalize_last(inter[-1])[1]
        return out

    pre, main, final = K.host_statement(states)
    assert np.array_equal(final, M.keccak_f(states))
    ok = claimed(pre, main)
    assert K.total(ok) == [0, 0, 0, 0] and all(ok[name].any() for name in K.COMPONENTS)
    main[200] = main[200].copy()
    main[200][0] ^= 1
    assert K.total(claimed(pre, main)) != [0, 0, 0, 0]
