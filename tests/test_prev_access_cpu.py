"""nx_trace_prev_access, what needs no GPU: the export and its mirrors (Python structures, generated -sys crate, hand-written Rust
wrapper), every refusal with a NULL context, the kernels themselves compiled as host C++ and run in lock step under the sanitizers
(tests/native/prev_access_emul.cpp), and the sequential model against a register trace written out by hand."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

import prev_access_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX_ERR_ARG = -2
P = M.P


def _lib():
    import nexus_zkvm_amd as nz
    if not os.path.exists(nz.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nz, nz.load_library()


def test_symbol_is_declared_exported_and_mirrored():
    nz, lib = _lib()
    assert "nx_trace_prev_access" in nz.declared_symbols()
    assert hasattr(lib, "nx_trace_prev_access")
    assert hasattr(nz.HipBackend, "trace_prev_access")
    # struct sizes as a C compiler lays the header's declarations out (LP64: 5 pointers + 3 words, padded; 1 word, padded, 3 pointers)
    assert C.sizeof(nz.AccessStream) == 56 and C.sizeof(nz.AccessSummary) == 32
    header = open(nz.HEADER_PATH).read()
    for name, cls in (("nx_access_stream", nz.AccessStream), ("nx_access_summary", nz.AccessSummary)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f for f, _ in cls._fields_], (names, cls._fields_)


def test_struct_sizes_are_the_compilers(tmp_path):
    gxx = shutil.which("g++")
    src = tmp_path / "sizes.cpp"
    src.write_text('#include "nexus_hip.h"\n#include <cstdio>\n#include <cstddef>\nint main() { printf("%zu %zu %zu %zu\\n", sizeof(nx_access_stream), sizeof(nx_access_summary), '
                   'offsetof(nx_access_stream, log_size), offsetof(nx_access_summary, d_key)); }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run([gxx, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    nz, _ = _lib()
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(nz.AccessStream), C.sizeof(nz.AccessSummary), nz.AccessStream.log_size.offset, nz.AccessSummary.d_key.offset]


def test_sys_crate_is_the_generators_output_and_the_wrapper_calls_it():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sys_src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct nx_access_stream \{(.*?)\n\}", sys_src, flags=re.S).group(1)
    assert re.findall(r"^\s*pub (\w+):", body, flags=re.M) == ["d_key", "d_flag", "d_payload", "d_prev", "d_ordinal", "log_size", "epoch", "linear"]
    body = re.search(r"pub struct nx_access_summary \{(.*?)\n\}", sys_src, flags=re.S).group(1)
    assert re.findall(r"^\s*pub (\w+):", body, flags=re.M) == ["cap", "d_key", "d_count", "d_last"]
    assert "pub fn nx_trace_prev_access(ctx: *mut nx_ctx, streams: *const nx_access_stream, n_streams: u32, n_key_cols: u32, key_bits: *const u32, n_payload: u32, " \
           "init: *const u32, summary: *const nx_access_summary, n_keys: *mut u64) -> c_int;" in sys_src
    hip = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "lib.rs")).read()
    assert "pub unsafe fn trace_prev_access(&mut self" in hip and "sys::nx_trace_prev_access(" in hip


class _Call:
    """A well-formed call made of host-only pointers that are never followed (the context is NULL), one piece of which a test breaks."""

    def __init__(self, nz, lib, n_streams=2, key_bits=(8, 5), n_payload=3):
        self.nz, self.f = nz, lib.nx_trace_prev_access
        self.f.restype = C.c_int
        self.f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib, self.keep, self.next = lib, [], 0x10000
        self.bits = (C.c_uint32 * 4)(*(list(key_bits) + [1] * (4 - len(key_bits))))
        self.k, self.np = len(key_bits), n_payload
        self.streams = (nz.AccessStream * max(1, n_streams))()
        for i in range(n_streams):
            self.streams[i] = nz.AccessStream(self.table(self.k), self.ptr(), self.table(n_payload), self.table(n_payload), self.ptr(), 4, 0, 0)
        self.n_streams = n_streams
        self.init = (C.c_uint32 * 16)(*([P - 1] * 16))
        self.summary = nz.AccessSummary(8, self.ptr(), self.ptr(), self.table(n_payload))

    def ptr(self):
        self.next += 0x1000
        return self.next

    def table(self, n, values=None):
        t = (C.c_void_p * max(1, n))(*(values if values is not None else [self.ptr() for _ in range(n)]))
        self.keep.append(t)
        return C.cast(t, C.c_void_p).value

    def __call__(self, streams=True, bits=True, n_streams=None, k=None, n_payload=None, init=True, summary=True):
        n_keys = C.c_uint64(77)
        rc = self.f(None, C.addressof(self.streams) if streams else None, self.n_streams if n_streams is None else n_streams, self.k if k is None else k,
                    C.addressof(self.bits) if bits else None, self.np if n_payload is None else n_payload, C.addressof(self.init) if init else None,
                    C.addressof(self.summary) if summary else None, C.byref(n_keys))
        assert n_keys.value == 77                    # the output scalar is left alone by every refusal
        return rc, self.lib.nx_last_error(None).decode()


def test_every_refusal_is_reached_with_a_null_context_and_names_its_argument():
    nz, lib = _lib()

    def refused(text, build=lambda c: None, **kw):
        c = _Call(nz, lib)
        build(c)
        rc, msg = c(**kw)
        assert rc == NX_ERR_ARG and msg.startswith("nx_trace_prev_access: ") and text in msg, (rc, msg, text)

    refused("NULL context")                                         # everything else well formed
    refused("NULL streams", streams=False)
    refused("NULL key_bits", bits=False)
    refused("n_streams of 0", n_streams=0)
    refused("n_streams of 65537", n_streams=65537)
    refused("n_key_cols of 0", k=0)
    refused("n_key_cols of 5", k=5)
    refused("n_payload of 0", n_payload=0)
    refused("n_payload of 17", n_payload=17)
    refused("key_bits[1] of 0", lambda c: c.bits.__setitem__(1, 0))
    refused("key_bits[0] of 33", lambda c: c.bits.__setitem__(0, 33))
    refused("add up to more than 32", lambda c: (c.bits.__setitem__(0, 20), c.bits.__setitem__(1, 13)))
    refused("init[2] is not below p", lambda c: c.init.__setitem__(2, P))
    refused("stream 1: log_size of 0", lambda c: setattr(c.streams[1], "log_size", 0))
    refused("stream 0: log_size of 31", lambda c: setattr(c.streams[0], "log_size", 31))
    refused("stream 1: log_size of 31", lambda c: (setattr(c.streams[1], "log_size", 31), setattr(c.streams[1], "linear", 1)))
    refused("2^31 rows or more", lambda c: (setattr(c.streams[0], "log_size", 30), setattr(c.streams[1], "log_size", 30)))
    refused("stream 1: NULL d_key", lambda c: setattr(c.streams[1], "d_key", None))
    refused("stream 0: NULL d_key[1]", lambda c: setattr(c.streams[0], "d_key", c.table(2, [0x500000, None])))
    # an output pointer that some other column of the call has: an input, another output, a summary array
    refused("output column", lambda c: setattr(c.streams[1], "d_ordinal", c.streams[0].d_flag))
    refused("output column", lambda c: setattr(c.streams[1], "d_ordinal", c.streams[0].d_ordinal))
    refused("output column", lambda c: setattr(c.streams[0], "d_prev", c.streams[0].d_payload))
    refused("output column", lambda c: setattr(c.summary, "d_count", c.summary.d_key))
    refused("output column", lambda c: setattr(c.summary, "d_key", c.streams[1].d_ordinal))
    # not refused for their own sake: a linear stream of one row, a stream that wants no output, no init, no summary — the NULL context is
    # all that is left to object to
    refused("NULL context", lambda c: (setattr(c.streams[0], "log_size", 0), setattr(c.streams[0], "linear", 1)))
    refused("NULL context", lambda c: (setattr(c.streams[0], "d_prev", None), setattr(c.streams[0], "d_ordinal", None), setattr(c.streams[0], "d_payload", None)))
    refused("NULL context", init=False, summary=False)
    assert lib.nx_trace_prev_access(None, None, 0, 0, None, 0, None, None, None) == NX_ERR_ARG


def test_coset_row_mapping_has_one_text():
    """pos_of_coset_row / coset_row_of_pos live in csrc/trace_rows.h alone: the kernels compiled ahead of time include it as code, the
    preludes of the generated kernels take it as text.  In the same way what nx_trace_prev_access and nx_trace_access_chain share lives in
    csrc/access_history.cuh alone: the time-index formula, the sort policy and the quad load of the resolve are defined there and in no
    other file, and the two entries' files include it."""
    csrc = os.path.join(ROOT, "nexus-zkvm_amd", "csrc")
    one_text = {"pos_of_coset_row": r"u32 pos_of_coset_row\(u32 \w+, int log\) \{", "coset_row_of_pos": r"u32 coset_row_of_pos\(u32 \w+, int log\) \{",
                "time index": r"u32 \w*time_index\([^)]*\) \{", "the formula itself": r"\+ r \* \w+(?:->|\.)ge\[b\] \+", "sort policy": r"struct \w+Sort \{\s*const u32\* kin; const u32\* vin; u32\* kout; u32\* vout; \w+Pass ps;",
                "load_quad": r"void \w*load_quad\([^)]*\) \{"}
    defs = {}
    for name in sorted(os.listdir(csrc)) + ["host/" + n for n in sorted(os.listdir(os.path.join(csrc, "host")))]:
        if os.path.isfile(os.path.join(csrc, name)) and name.endswith((".hip", ".h", ".cuh", ".cpp")):
            text = open(os.path.join(csrc, name)).read()
            for what, pattern in one_text.items():
                defs.setdefault(what, []).extend([name] * len(re.findall(pattern, text)))
    assert defs == {"pos_of_coset_row": ["trace_rows.h"], "coset_row_of_pos": ["trace_rows.h"], "time index": ["access_history.cuh"],
                    "the formula itself": ["access_history.cuh"], "sort policy": ["access_history.cuh"], "load_quad": ["access_history.cuh"]}, defs
    for user in ("air_jit.hip", "logup.hip", "access_history.cuh"):
        assert '#include "trace_rows.h"' in open(os.path.join(csrc, user)).read()
    for user in ("prev_access.hip", "access_chain.hip"):
        text = open(os.path.join(csrc, user)).read()
        assert '#include "access_history.cuh"' in text and "__global__" not in text and "struct " not in text, user


def test_both_readers_of_the_coset_row_text_compute_the_models_mapping(tmp_path):
    """csrc/trace_rows.h as code (what logup.hip and access_history.cuh compile) and as the text inside a generated kernel's source (what
    hiprtc compiles), both built as host C++: the same rows as the model's definition at every position of 2^1 .. 2^10 rows, and
    pos_of_coset_row is the inverse."""
    nz, _ = _lib()
    import nexus_zkvm_amd.air_program as ap
    pb = ap.ProgramBuilder()
    pb.store(0, pb.row())
    generated = nz.trace_program_source(pb.build_trace_program(), 1)
    line = [l for l in generated.split("\n") if "FI u32 pos_of_coset_row(" in l and "FI u32 coset_row_of_pos(" in l]
    assert len(line) == 1, "the generated source carries the two functions once, on the line the header was stringified to"
    src = tmp_path / "rows.cpp"
    src.write_text("#include <cstdint>\n#include <cstdio>\ntypedef uint32_t u32;\n"
                   "static inline u32 bitrev(u32 i, int log) { u32 r = 0; for (int b = 0; b < log; b++) r |= ((i >> b) & 1u) << (log - 1 - b); return r; }\n"
                   "#define NX_HD static inline\nnamespace code {\n#include \"trace_rows.h\"\n}\n#define FI static inline\nnamespace text {\n" + line[0] + "\n}\n"
                   "int main() { for (int log = 1; log <= 10; log++) for (u32 p = 0; p < (1u << log); p++) {\n"
                   "  const u32 r = code::coset_row_of_pos(p, log);\n"
                   "  if (r != text::coset_row_of_pos(p, log) || code::pos_of_coset_row(r, log) != p || text::pos_of_coset_row(r, log) != p) { printf(\"differ at %d %u\\n\", log, p); return 1; }\n"
                   "  printf(\"%u\\n\", r); } return 0; }\n")
    exe = str(tmp_path / "rows")
    subprocess.run([shutil.which("g++"), "-std=c++17", "-I" + os.path.join(ROOT, "nexus-zkvm_amd", "csrc"), str(src), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-300:]
    assert [int(x) for x in r.stdout.split()] == [M.coset_row_of_pos(p, log) for log in range(1, 11) for p in range(1 << log)]


def test_kernels_in_lock_step_on_the_host_under_sanitizers(tmp_path):
    """csrc/prev_access.hip with csrc/access_history.cuh as host C++ (tests/native/prev_emul/internal.h: 256 lock-step fibers per block, waves of 64): every key
    shape, stream count, size up to 2^12 rows, flag / ordinal / summary / NULL-column choice, the skewed inputs, epochs and mixed
    sizes, short summaries, rows out of range (also refused rows sorted between real keys) and a refusal against a walk over a map, with ASan and UBSan watching every LDS,
    histogram, placement and summary index — and the device-memory bound of the header.  Twice: as built, and with a block cap of 2,
    where a block of the sort takes up to eight tiles and the case of 2^11 + 2 elements takes five in each of its two passes."""
    gxx = shutil.which("g++")
    native = os.path.join(ROOT, "tests", "native")
    csrc = os.path.join(ROOT, "nexus-zkvm_amd", "csrc")
    shutil.copy(os.path.join(csrc, "prev_access.hip"), str(tmp_path / "prev_access_emu.cpp"))
    shutil.copy(os.path.join(csrc, "trace_rows.h"), str(tmp_path / "trace_rows.h"))
    shutil.copy(os.path.join(csrc, "count_pass.cuh"), str(tmp_path / "count_pass.cuh"))
    shutil.copy(os.path.join(csrc, "access_history.cuh"), str(tmp_path / "access_history.cuh"))
    shutil.copy(os.path.join(native, "prev_emul", "internal.h"), str(tmp_path / "internal.h"))
    for cap, flags in ((1024, []), (2, ["-DNX_COUNT_PASS_MAX_BLOCKS=2"])):
        exe = str(tmp_path / ("prev_access_emul_%d" % cap))
        subprocess.run([gxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-Wno-unknown-pragmas"] + flags +
                       ["-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"), os.path.join(native, "prev_access_emul.cpp"), "-o", exe], check=True, capture_output=True)
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "\n0 failures" in r.stdout and r.stdout.count(" OK ") >= 71 and "FAIL" not in r.stdout and ("block cap %d\n" % cap) in r.stdout
        assert "linear streams of 2^11 and 2 rows " in r.stdout and "PLAN NOT REACHED" not in r.stdout
        assert "refused rows between keys of digit 255, one pass " in r.stdout and "refused rows between keys of digit 255, four passes " in r.stdout
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def _same_answers(a, b):
    assert a["bad"] == b["bad"]
    for name in ("keys", "counts"):
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name
    assert len(a["last"]) == len(b["last"]) and all(np.array_equal(x, y) for x, y in zip(a["last"], b["last"]))
    assert len(a["prev"]) == len(b["prev"])
    for s in range(len(a["prev"])):
        assert np.array_equal(a["ordinal"][s], b["ordinal"][s]), s
        assert len(a["prev"][s]) == len(b["prev"][s]) and all(np.array_equal(x, y) for x, y in zip(a["prev"][s], b["prev"][s])), s


def test_the_model_by_sorting_is_the_sequential_model():
    """M.model_by_sorting, the judge of the device case of 2^20 rows, against the dictionary walk: that case's own shape at 2^11 rows (M.two_linear_streams),
    and epochs, mixed sizes, bit-reversed streams, flags, NULL payload columns and rows out of their bits"""
    streams = M.two_linear_streams(np.random.default_rng(2011), 11)
    assert [(s["log_size"], s["linear"], s["flag"] is not None) for s in streams] == [(11, True, True), (1, True, False)]
    init = [P - 3]
    _same_answers(M.model_by_sorting(streams, [8, 5], 1, init), M.model(streams, [8, 5], 1, init))
    rng = np.random.default_rng(2012)
    mixed = []
    for log, epoch, linear, flags in ((7, 0, True, False), (9, 1, False, True), (9, 1, False, False), (6, 1, False, True), (0, 1, True, False), (3, 7, False, False)):
        n = 1 << log
        mixed.append({"key": [rng.integers(0, 256, n, dtype=np.uint32), rng.integers(0, 4, n, dtype=np.uint32)], "flag": rng.integers(0, 3, n, dtype=np.uint32) if flags else None,
                      "payload": [rng.integers(0, P, n, dtype=np.uint32), None, rng.integers(0, P, n, dtype=np.uint32)], "log_size": log, "epoch": epoch, "linear": linear})
    _same_answers(M.model_by_sorting(mixed, [8, 5], 3, [1, 2, 3]), M.model(mixed, [8, 5], 3, [1, 2, 3]))
    _same_answers(M.model_by_sorting(mixed, [8, 5], 3), M.model(mixed, [8, 5], 3))
    mixed[2]["key"][1][300] = 32                                     # outside its 5 bits on rows that access: skipped and named
    mixed[1]["key"][0][17], mixed[1]["flag"][17] = 256, 2
    mixed[1]["key"][0][5], mixed[1]["flag"][5] = 999, 0              # and on one that does not: ignored
    want = M.model(mixed, [8, 5], 3)
    assert want["bad"] == (1, 17)
    _same_answers(M.model_by_sorting(mixed, [8, 5], 3), want)


def test_model_reproduces_the_register_trace_written_out_by_hand():
    """32 keys, three streams per row in slot order, timestamps 3 clk + slot, init 0: tests/golden/register_prev_access.json holds the
    Reg{1,2,3}TsPrev / ValPrev columns and the final register state of a small add chain, derived by hand from the register chip's rule."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "register_prev_access.json")))
    log = g["log_size"]
    n = 1 << log
    col = lambda a: M.to_storage(np.array(a, np.uint32), log)
    for slot, s in enumerate(g["slots"], start=1):
        assert s["ts"] == [3 * (row + 1) + slot for row in range(n)]
    streams = [{"key": [col(s["address"])], "flag": col(s["accessed"]), "payload": [col(s["ts"]), col(s["value"])], "log_size": log} for s in g["slots"]]
    r = M.model(streams, [5], 2, init=[0, 0])
    for i, s in enumerate(g["slots"]):
        assert np.array_equal(r["prev"][i][0], col(s["ts_prev"])) and np.array_equal(r["prev"][i][1], col(s["val_prev"])), i
        assert np.array_equal(r["ordinal"][i], col(s["ordinal"])), i
    f = g["final"]
    assert (r["keys"].tolist(), r["counts"].tolist(), r["last"][0].tolist(), r["last"][1].tolist()) == (f["register"], f["accesses"], f["ts"], f["value"])
    assert r["bad"] is None
