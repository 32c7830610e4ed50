"""nx_trace_partition_create / _fill, what needs no GPU: the model of tests/trace_partition_model.py against a ten-step table written
out by hand, the exports and their mirrors (Python structures against the compiler's layout, generated -sys crate, hand-written Rust
wrapper, documents), every refusal that can be met with a NULL context, and the kernels themselves compiled as host C++ and run in
lock step under the sanitizers as a program of its own (tests/native/trace_partition_emul.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np

import trace_partition_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX_ERR_ARG = -2
P = M.P


def _lib():
    import nexus_zkvm_amd as nz
    if not os.path.exists(nz.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nz, nz.load_library()


def test_model_on_a_ten_step_table_written_out_by_hand():
    """classes 0 1 0 2 - 1 0 0 2 1 (- = in no component); source word 0x01020300 + step.  The rows of a 4-row column sit at storage
    positions 0 3 2 1, those of a 16-row column at 0 15 8 7 4 11 12 3 2 13 10 5 6 9 14 1."""
    cls = np.array([0, 1, 0, 2, M.NONE, 1, 0, 0, 2, 1], np.uint32)
    src = [np.arange(10, dtype=np.uint32) + 0x01020300]
    counts, steps = M.partition(cls, 3)
    assert counts.tolist() == [4, 3, 2]
    assert [s.tolist() for s in steps] == [[0, 2, 6, 7], [1, 5, 9], [3, 8]]
    assert [M.log_size(c, 1) for c in counts] == [2, 2, 1] and [M.log_size(c, 4) for c in (0, 1, 16, 17)] == [4, 4, 4, 5] and M.log_size(0, 0) == 0
    assert M.rows_of_positions(2).tolist() == [0, 3, 2, 1]
    assert M.rows_of_positions(4).tolist() == [0, 15, 8, 7, 4, 11, 12, 3, 2, 13, 10, 5, 6, 9, 14, 1]
    r = M.fill(cls, 3, src, {"cls": 0, "log_size": 2, "limbs": [(0, 0, 8)]})
    assert r["step"].tolist() == [0, 7, 6, 2] and r["is_pad"].tolist() == [0, 0, 0, 0] and r["cols"][0].tolist() == [0, 7, 6, 2]
    r = M.fill(cls, 3, src, {"cls": 1, "log_size": 2, "limbs": [(0, 0, 8), (0, 8, 8), (0, 16, 16), (0, 0, 1)]})
    assert r["step"].tolist() == [1, 0, 9, 5] and r["is_pad"].tolist() == [0, 1, 0, 0]
    assert [c.tolist() for c in r["cols"]] == [[1, 0, 9, 5], [3, 0, 3, 3], [0x0102, 0, 0x0102, 0x0102], [1, 0, 1, 1]]
    r = M.fill(cls, 3, src, {"cls": 2, "log_size": 3, "limbs": [(0, 2, 6)]})         # rows 0 7 4 3 2 5 6 1: two steps, six padding rows
    assert r["step"].tolist() == [3, 0, 0, 0, 0, 0, 0, 8] and r["is_pad"].tolist() == [0, 1, 1, 1, 1, 1, 1, 0] and r["cols"][0].tolist() == [0, 0, 0, 0, 0, 0, 0, 2]
    r = M.fill(cls, 3, src, {"cls": M.ALL, "log_size": 4, "limbs": [(0, 0, 8)]})
    assert r["step"].tolist() == [0, 0, 8, 7, 4, 0, 0, 3, 2, 0, 0, 5, 6, 9, 0, 1] == r["cols"][0].tolist()
    assert r["is_pad"].tolist() == [0, 1, 0, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0]
    assert M.first_bad(cls, 3) is None and M.first_bad(np.array([0, 3, 5, M.NONE], np.uint32), 3) == (1, 3)
    # the value p is written as 0; 31 bits above bit 0 are not
    assert M.limb(P, 0, 31) == 0 and M.limb(0xFFFFFFFF, 0, 31) == 0 and M.limb(0xFFFFFFFF, 1, 31) == 0 and M.limb(0xFFFFFFFE, 1, 31) == 0 and M.limb(0xFFFFFFFD, 1, 31) == P - 1
    assert M.limb(0x80000000, 31, 1) == 1 and M.limb(0x7FFFFFFF, 31, 1) == 0


def test_the_models_array_forms_are_its_scalar_definitions():
    for log in range(1, 9):                                  # a trace column has at least two rows
        assert M.rows_of_positions(log).tolist() == [M.coset_row_of_pos(p, log) for p in range(1 << log)]
        assert sorted(M.rows_of_positions(log).tolist()) == list(range(1 << log))
    rng = np.random.default_rng(3)
    words = np.concatenate([rng.integers(0, 1 << 32, size=200, dtype=np.uint64).astype(np.uint32), np.array([P, 0xFFFFFFFF, 0xFFFFFFFE, 0, 0x80000000], np.uint32)])
    for shift, bits in [(0, 8), (8, 8), (16, 16), (2, 6), (0, 1), (31, 1), (0, 31), (1, 31), (24, 8), (5, 27)]:
        assert M.limbs_of(words, shift, bits).tolist() == [M.limb(w, shift, bits) for w in words.tolist()]


def test_symbols_are_declared_exported_and_mirrored():
    nz, lib = _lib()
    names = ("nx_trace_partition_create", "nx_trace_partition_log_size", "nx_trace_partition_fill", "nx_trace_partition_destroy")
    for name in names:
        assert name in nz.declared_symbols() and hasattr(lib, name), name
    assert hasattr(nz.HipBackend, "trace_partition") and hasattr(nz.TracePartition, "fill") and hasattr(nz.TracePartition, "destroy")
    assert (nz.PART_NONE, nz.PART_ALL, nz.PART_MAX_CLASSES) == (0xFFFFFFFF, 0xFFFFFFFF, 256)
    header = open(nz.HEADER_PATH).read()
    assert "#define NX_PART_NONE 0xFFFFFFFFu" in header and "#define NX_PART_ALL  0xFFFFFFFFu" in header and "#define NX_PART_MAX_CLASSES 256" in header
    for name, cls in (("nx_part_limb", nz.PartLimb), ("nx_part_dest", nz.PartDest)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert fields == [f for f, _ in cls._fields_], (fields, cls._fields_)
    doc = header[header.index("the step table split into per-opcode"):header.index("int nx_trace_partition_create")]
    for needle in ("execution/common/mod.rs:31-39", "execution/add/mod.rs:", "components/cpu/trace.rs:36-59", "NX_ERR_PROTOCOL", "DEVICE MEMORY", "bit-reversed circle-domain order"):
        assert needle in doc, needle
    for path in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, path)).read()
        assert "nx_trace_partition_create" in text and "nx_trace_partition_fill" in text, path
    assert "iter_program_steps" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "trace_partition.hip" in open(os.path.join(ROOT, "nexus-zkvm_amd", "csrc", "Makefile")).read()


def test_struct_sizes_and_offsets_are_the_compilers(tmp_path):
    gxx = shutil.which("g++")
    src = tmp_path / "sizes.cpp"
    src.write_text('#include "nexus_hip.h"\n#include <cstdio>\n#include <cstddef>\nint main() { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(nx_part_limb), '
                   'offsetof(nx_part_limb, shift), offsetof(nx_part_limb, bits), sizeof(nx_part_dest), offsetof(nx_part_dest, log_size), offsetof(nx_part_dest, n_cols), '
                   'offsetof(nx_part_dest, d_cols), offsetof(nx_part_dest, limbs), offsetof(nx_part_dest, d_is_pad), offsetof(nx_part_dest, d_step)); }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run([gxx, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    nz, _ = _lib()
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    L, D = nz.PartLimb, nz.PartDest
    assert got == [C.sizeof(L), L.shift.offset, L.bits.offset, C.sizeof(D), D.log_size.offset, D.n_cols.offset, D.d_cols.offset, D.limbs.offset, D.d_is_pad.offset, D.d_step.offset]
    assert got[0] == 12 and got[3] == 48


def test_sys_crate_is_the_generators_output_and_the_wrapper_calls_it():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sys_src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    assert "pub struct nx_partition { _private: [u8; 0] }" in sys_src
    body = re.search(r"pub struct nx_part_limb \{(.*?)\n\}", sys_src, flags=re.S).group(1)
    assert re.findall(r"^\s*pub (\w+):", body, flags=re.M) == ["src", "shift", "bits"]
    body = re.search(r"pub struct nx_part_dest \{(.*?)\n\}", sys_src, flags=re.S).group(1)
    assert re.findall(r"^\s*pub (\w+):", body, flags=re.M) == ["cls", "log_size", "n_cols", "d_cols", "limbs", "d_is_pad", "d_step"]
    assert "pub fn nx_trace_partition_create(ctx: *mut nx_ctx, d_class: *const u32, n_steps: u32, n_classes: u32, counts: *mut u32, out: *mut *mut nx_partition) -> c_int;" in sys_src
    assert "pub fn nx_trace_partition_log_size(count: u64, min_log: u32) -> u32;" in sys_src
    assert "pub fn nx_trace_partition_fill(ctx: *mut nx_ctx, part: *const nx_partition, d_src: *const *const u32, n_src: u32, dests: *const nx_part_dest, n_dests: u32) -> c_int;" in sys_src
    assert "pub fn nx_trace_partition_destroy(part: *mut nx_partition);" in sys_src
    hip = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "lib.rs")).read()
    for needle in ("pub unsafe fn trace_partition(&mut self", "sys::nx_trace_partition_create(", "pub unsafe fn trace_partition_fill(&mut self", "sys::nx_trace_partition_fill(",
                   "sys::nx_trace_partition_destroy(", "sys::nx_trace_partition_log_size("):
        assert needle in hip, needle


def test_log_size_helper_is_pure_host_arithmetic():
    nz, lib = _lib()
    for count in [0, 1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, (1 << 30) - 1, 1 << 30, (1 << 30) + 1]:
        for min_log in (0, 1, 4, 31):
            assert nz.partition_log_size(count, min_log) == M.log_size(count, min_log), (count, min_log)


def test_refusals_that_need_no_device_name_their_argument():
    nz, lib = _lib()
    f = lib.nx_trace_partition_create
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    counts = (C.c_uint32 * 256)(*([77] * 256))
    CLS = 0x10000                     # a pointer that is never followed: the context is NULL

    def refused(text, cls=CLS, n_steps=100, n_classes=40, with_counts=True, with_out=True):
        out = C.c_void_p(0x55)
        rc = f(None, cls, n_steps, n_classes, C.addressof(counts) if with_counts else None, C.byref(out) if with_out else None)
        msg = lib.nx_last_error(None).decode()
        assert rc == NX_ERR_ARG and msg.startswith("nx_trace_partition_create: ") and text in msg, (rc, msg, text)
        assert out.value == 0x55 and all(c == 77 for c in counts)           # the outputs are left alone by every refusal

    refused("NULL context")                                                # everything else well formed
    refused("NULL context", cls=None, n_steps=0)                           # an empty table needs no class column
    refused("NULL out", with_out=False)
    refused("NULL counts", with_counts=False)
    refused("n_classes of 0", n_classes=0)
    refused("n_classes of 257", n_classes=257)
    refused("n_steps of 1073741825", n_steps=(1 << 30) + 1)
    refused("NULL context", n_steps=1 << 30, n_classes=256)
    refused("NULL d_class with n_steps of 100", cls=None)
    g = lib.nx_trace_partition_fill
    g.restype = C.c_int
    g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    assert g(None, None, None, 0, None, 0) == NX_ERR_ARG and "nx_trace_partition_fill: NULL partition" in lib.nx_last_error(None).decode()
    lib.nx_trace_partition_destroy(None)                                   # a no-op


def test_kernels_in_lock_step_on_the_host_under_sanitizers(tmp_path):
    """csrc/trace_partition.hip as host C++ (tests/native/prev_emul/internal.h: 256 lock-step fibers per block, waves of 64;
    tests/native/part_emul/shim.h on top): the sizes around every tile edge, 1 / 3 / 40 / 256 classes, every skew, every limb shape,
    destinations for every class and for all steps, the optional outputs, both refused class words and every NX_ERR_ARG of the fill
    against a sequential filter-and-enumerate walk, guard words behind every output, with ASan and UBSan watching every LDS, histogram,
    order and descriptor index.  Twice: as built, and with a block cap of 2, where a block of the counting pass takes seven tiles."""
    gxx = shutil.which("g++")
    native = os.path.join(ROOT, "tests", "native")
    csrc = os.path.join(ROOT, "nexus-zkvm_amd", "csrc")
    shutil.copy(os.path.join(csrc, "trace_partition.hip"), str(tmp_path / "trace_partition_emu.cpp"))
    shutil.copy(os.path.join(csrc, "trace_rows.h"), str(tmp_path / "trace_rows.h"))
    shutil.copy(os.path.join(csrc, "count_pass.cuh"), str(tmp_path / "count_pass.cuh"))
    shutil.copy(os.path.join(native, "prev_emul", "internal.h"), str(tmp_path / "internal.h"))
    shutil.copy(os.path.join(native, "part_emul", "shim.h"), str(tmp_path / "shim.h"))
    for cap, flags in ((1024, []), (2, ["-DNX_COUNT_PASS_MAX_BLOCKS=2"])):
        exe = str(tmp_path / ("trace_partition_emul_%d" % cap))
        subprocess.run([gxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-Wno-unknown-pragmas"] + flags +
                       ["-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"), os.path.join(native, "trace_partition_emul.cpp"), "-o", exe], check=True, capture_output=True)
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "\n0 failures" in r.stdout and r.stdout.count(" OK ") >= 90 and "FAIL" not in r.stdout and ("block cap %d\n" % cap) in r.stdout
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
