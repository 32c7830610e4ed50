"""nx_logup_multiplicities, what needs no GPU: the export, its refusals with a NULL context, the constant the GPU tests read the LDS
cut-off from, the Rust binding (generated -sys crate, hand-written wrapper) — and the kernels themselves, compiled as host C++ and run
in lock step under the sanitizers (tests/native/multiplicity_emul.cpp)."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX_ERR_ARG = -2


def _lib():
    import nexus_zkvm_amd as nz
    if not os.path.exists(nz.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nz, nz.load_library()


def test_symbol_is_declared_and_exported():
    nz, lib = _lib()
    assert "nx_logup_multiplicities" in nz.declared_symbols()
    assert hasattr(lib, "nx_logup_multiplicities")
    assert hasattr(nz.HipBackend, "logup_multiplicities")


def test_lds_cut_off_constant_is_the_headers():
    nz, _ = _lib()
    m = re.search(r"^#define NX_MULT_LDS_MAX_KEY_BITS (\d+)\s*$", open(nz.HEADER_PATH).read(), flags=re.M)
    assert m and int(m.group(1)) == nz.MULT_LDS_MAX_KEY_BITS
    assert 4 <= nz.MULT_LDS_MAX_KEY_BITS < 24        # both forms exist below the 24-bit key limit
    src = open(os.path.join(ROOT, "nexus-zkvm_amd", "csrc", "multiplicity.hip")).read()
    assert "NX_MULT_LDS_MAX_KEY_BITS" in src


def test_argument_errors_with_a_null_context_are_errors_not_crashes():
    """ctx == NULL is NX_ERR_ARG whatever else is passed — all NULL, or every other argument well formed (host-side pointers that are
    never followed) — and the outputs are left alone."""
    nz, lib = _lib()
    f = lib.nx_logup_multiplicities
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert f(None, None, 0, 0, None, None, 0, None, None, None, None) == NX_ERR_ARG
    assert b"nx_logup_multiplicities" in lib.nx_last_error(None)
    bits = (C.c_uint32 * 2)(8, 8)
    vals = (C.c_void_p * 2)(0x1000, 0x2000)
    use = nz.LookupUse(C.cast(vals, C.c_void_p), None, 4)
    table = (C.c_void_p * 2)(0x3000, 0x4000)
    n, fu, fp = C.c_uint64(77), C.c_uint32(78), C.c_uint64(79)
    assert f(None, C.byref(use), 1, 2, bits, table, 16, C.c_void_p(0x5000), C.byref(n), C.byref(fu), C.byref(fp)) == NX_ERR_ARG
    assert (n.value, fu.value, fp.value) == (77, 78, 79)
    assert f(None, C.byref(use), 1, 5, bits, table, 16, C.c_void_p(0x5000), None, None, None) == NX_ERR_ARG
    assert C.sizeof(nz.LookupUse) == 24


def test_sys_crate_is_the_generators_output_and_the_wrapper_calls_it():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sys_src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct nx_lookup_use \{(.*?)\n\}", sys_src, flags=re.S).group(1)
    assert re.findall(r"^\s*pub (\w+):", body, flags=re.M) == ["d_values", "d_weight", "log_size"]
    assert "pub fn nx_logup_multiplicities(ctx: *mut nx_ctx, uses: *const nx_lookup_use," in sys_src
    hip = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "lib.rs")).read()
    assert "pub fn logup_multiplicities(&mut self" in hip and "sys::nx_logup_multiplicities(" in hip


def test_kernels_in_lock_step_on_the_host_under_sanitizers(tmp_path):
    """csrc/multiplicity.hip as host C++ (tests/native/mult_emul/internal.h: 256 lock-step threads per block, waves of 64): every counting
    form, table order, weight kind, missing row and refusal against a brute-force count, with ASan and UBSan watching every LDS and
    counter index."""
    import shutil
    gxx = shutil.which("g++")
    native = os.path.join(ROOT, "tests", "native")
    shutil.copy(os.path.join(ROOT, "nexus-zkvm_amd", "csrc", "multiplicity.hip"), str(tmp_path / "multiplicity_emu.cpp"))
    shutil.copy(os.path.join(native, "mult_emul", "internal.h"), str(tmp_path / "internal.h"))
    exe = str(tmp_path / "multiplicity_emul")
    subprocess.run([gxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-Wno-unknown-pragmas",
                    "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"), os.path.join(native, "multiplicity_emul.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "\n0 failures" in r.stdout and r.stdout.count(" OK ") >= 50 and "FAIL" not in r.stdout
