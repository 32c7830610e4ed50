"""nx_trace_access_chain, what needs no GPU: the export and its mirrors (Python structure, generated -sys crate, hand-written Rust
wrapper), the struct's layout against a compiler's, every NX_ERR_ARG refusal with a NULL context, the kernels themselves compiled as
host C++ and run in lock step under the sanitizers (tests/native/access_chain_emul.cpp), the array twin of the model against the walk,
and the walk against a RAM history written out by hand."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

import access_chain_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX_ERR_ARG = -2
P = M.P
FIELDS = ["d_key", "d_flag", "d_row", "d_payload", "rule", "delta", "d_prev", "d_ordinal", "log_size", "n_records", "span", "epoch", "linear"]


def _lib():
    import nexus_zkvm_amd as nz
    if not os.path.exists(nz.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nz, nz.load_library()


def test_symbol_is_declared_exported_and_mirrored():
    nz, lib = _lib()
    assert "nx_trace_access_chain" in nz.declared_symbols()
    assert hasattr(lib, "nx_trace_access_chain")
    assert hasattr(nz.HipBackend, "trace_access_chain")
    assert (nz.CHAIN_GIVEN, nz.CHAIN_ADD, nz.CHAIN_BYTES) == (0, 1, 2) == (M.GIVEN, M.ADD, M.BYTES)
    header = open(nz.HEADER_PATH).read()
    for name, value in (("GIVEN", 0), ("ADD", 1), ("BYTES", 2)):
        assert re.search(r"^#define NX_CHAIN_%s\s+%du\b" % (name, value), header, flags=re.M), name
    body = re.search(r"typedef struct nx_chain_stream \{(.*?)\} nx_chain_stream;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == FIELDS == [f for f, _ in nz.ChainStream._fields_]
    assert C.sizeof(nz.ChainStream) == 88                          # LP64: 8 pointers, 5 words, padded


def test_struct_size_and_offsets_are_the_compilers(tmp_path):
    gxx = shutil.which("g++")
    src = tmp_path / "sizes.cpp"
    src.write_text('#include "nexus_hip.h"\n#include <cstdio>\n#include <cstddef>\nint main() { printf("%zu", sizeof(nx_chain_stream));\n' +
                   "".join('printf(" %%zu", offsetof(nx_chain_stream, %s));\n' % f for f in FIELDS) + 'printf("\\n"); }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run([gxx, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    nz, _ = _lib()
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(nz.ChainStream)] + [getattr(nz.ChainStream, f).offset for f in FIELDS]


def test_sys_crate_is_the_generators_output_and_the_wrapper_calls_it():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sys_src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct nx_chain_stream \{(.*?)\n\}", sys_src, flags=re.S).group(1)
    assert re.findall(r"^\s*pub (\w+):", body, flags=re.M) == FIELDS
    assert "pub d_row: *const u32," in body and "pub rule: *const u32," in body and "pub d_prev: *const *mut u32," in body
    assert "pub fn nx_trace_access_chain(ctx: *mut nx_ctx, streams: *const nx_chain_stream, n_streams: u32, n_key_cols: u32, key_bits: *const u32, n_payload: u32, " \
           "init: *const u32, summary: *const nx_access_summary, n_keys: *mut u64) -> c_int;" in sys_src
    hip = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "lib.rs")).read()
    assert "pub unsafe fn trace_access_chain(&mut self" in hip and "sys::nx_trace_access_chain(" in hip
    for name, value in (("GIVEN", 0), ("ADD", 1), ("BYTES", 2)):
        assert "pub const CHAIN_%s: u32 = %d;" % (name, value) in hip


class _Call:
    """A well-formed call made of host-only pointers that are never followed (the context is NULL), one piece of which a test breaks:
    stream 0 a column stream, stream 1 a block stream of 5 records of span 200 with (ADD, GIVEN | BYTES, GIVEN)."""

    def __init__(self, nz, lib, n_streams=2, key_bits=(8, 5), n_payload=3):
        self.nz, self.f = nz, lib.nx_trace_access_chain
        self.f.restype = C.c_int
        self.f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib, self.keep, self.next = lib, [], 0x10000
        self.bits = (C.c_uint32 * 4)(*(list(key_bits) + [1] * (4 - len(key_bits))))
        self.k, self.np = len(key_bits), n_payload
        self.streams = (nz.ChainStream * max(1, n_streams))()
        self.rule = (C.c_uint32 * 16)(*([nz.CHAIN_ADD, nz.CHAIN_GIVEN | nz.CHAIN_BYTES] + [nz.CHAIN_GIVEN] * 14))
        self.delta = (C.c_uint32 * 16)(*([1] * 16))
        for i in range(n_streams):
            if i == 1:
                pay = self.table(n_payload, [None] + [self.ptr() for _ in range(n_payload - 1)])
                self.streams[i] = nz.ChainStream(self.table(self.k), self.ptr(), self.ptr(), pay, C.addressof(self.rule), C.addressof(self.delta), self.table(n_payload), self.ptr(),
                                                 0, 5, 200, 0, 0)
            else:
                self.streams[i] = nz.ChainStream(self.table(self.k), self.ptr(), None, self.table(n_payload), None, None, self.table(n_payload), self.ptr(), 4, 0, 0, 0, 0)
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

    def words(self, values):
        t = (C.c_uint32 * len(values))(*values)
        self.keep.append(t)
        return C.addressof(t)

    def __call__(self, streams=True, bits=True, n_streams=None, k=None, n_payload=None, init=True, summary=True):
        n_keys = C.c_uint64(77)
        rc = self.f(None, C.addressof(self.streams) if streams else None, self.n_streams if n_streams is None else n_streams, self.k if k is None else k,
                    C.addressof(self.bits) if bits else None, self.np if n_payload is None else n_payload, C.addressof(self.init) if init else None,
                    C.addressof(self.summary) if summary else None, C.byref(n_keys))
        assert n_keys.value == 77                    # the output scalar is left alone by every refusal
        return rc, self.lib.nx_last_error(None).decode()


def test_every_refusal_is_reached_with_a_null_context_and_names_its_argument():
    nz, lib = _lib()

    def refused(text, build=lambda c: None, n=2, **kw):
        c = _Call(nz, lib, n_streams=n)
        build(c)
        rc, msg = c(**kw)
        assert rc == NX_ERR_ARG and msg.startswith("nx_trace_access_chain: ") and text in msg, (rc, msg, text)

    refused("NULL context")                                         # everything else well formed
    # what nx_trace_prev_access refuses
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
    refused("stream 0: log_size of 0", lambda c: setattr(c.streams[0], "log_size", 0))
    refused("stream 0: log_size of 31", lambda c: setattr(c.streams[0], "log_size", 31))
    refused("stream 0: log_size of 31", lambda c: (setattr(c.streams[0], "log_size", 31), setattr(c.streams[0], "linear", 1)))
    refused("stream 1: NULL d_key", lambda c: setattr(c.streams[1], "d_key", None))
    refused("stream 0: NULL d_key[1]", lambda c: setattr(c.streams[0], "d_key", c.table(2, [0x500000, None])))
    refused("output column", lambda c: setattr(c.streams[1], "d_ordinal", c.streams[0].d_flag))
    refused("output column", lambda c: setattr(c.streams[1], "d_ordinal", c.streams[0].d_ordinal))
    refused("output column", lambda c: setattr(c.streams[0], "d_prev", c.streams[0].d_payload))
    refused("output column", lambda c: setattr(c.streams[0], "d_ordinal", c.streams[1].d_row))
    refused("output column", lambda c: setattr(c.summary, "d_count", c.summary.d_key))
    refused("output column", lambda c: setattr(c.summary, "d_key", c.streams[1].d_ordinal))
    # 2^31 elements or more: rows of column streams plus n_records * span of block streams
    refused("2^31 elements or more", lambda c: (setattr(c.streams[0], "log_size", 30), setattr(c.streams[1], "n_records", 1 << 23), setattr(c.streams[1], "span", 128)))
    refused("2^31 elements or more", lambda c: (setattr(c.streams[1], "n_records", 0xFFFFFFFF), setattr(c.streams[1], "span", 256)))
    refused("2^31 elements or more", lambda c: (setattr(c.streams[0], "log_size", 30), setattr(c.streams[2], "log_size", 30)), n=3)
    # what is new
    refused("stream 1: span of 0", lambda c: setattr(c.streams[1], "span", 0))
    refused("stream 1: span of 257", lambda c: setattr(c.streams[1], "span", 257))

    def nine_block_streams(c):
        for i in range(1, 10):
            c.streams[i] = c.streams[1]
            c.streams[i].d_prev, c.streams[i].d_ordinal = None, None
    refused("stream 9: more than 8 block streams", nine_block_streams, n=10)
    refused("stream 0: rule[1]: NX_CHAIN_BYTES on a column stream", lambda c: setattr(c.streams[0], "rule", c.words([0, 2, 0])))
    refused("stream 1: rule[0]: NX_CHAIN_BYTES on an NX_CHAIN_ADD column", lambda c: setattr(c.streams[1], "rule", c.words([3, 2, 0])))
    refused("stream 1: rule[1]: NX_CHAIN_BYTES with a span of 6", lambda c: setattr(c.streams[1], "span", 6))
    refused("stream 1: rule[1]: NX_CHAIN_BYTES with a d_payload that is not 4-byte aligned", lambda c: setattr(c.streams[1], "d_payload", c.table(3, [None, 0x700002, 0x800000])))
    refused("stream 1: rule[2]: NX_CHAIN_ADD with a d_payload[2] that is not NULL", lambda c: setattr(c.streams[1], "rule", c.words([1, 2, 1])))
    refused("stream 0: rule[0]: NX_CHAIN_ADD with a d_payload[0] that is not NULL", lambda c: setattr(c.streams[0], "rule", c.words([1, 0, 0])))
    refused("stream 1: rule[2] of 4 is no rule", lambda c: setattr(c.streams[1], "rule", c.words([1, 2, 4])))
    refused("stream 0: rule[1] of 4294967295 is no rule", lambda c: setattr(c.streams[0], "rule", c.words([0, 0xFFFFFFFF, 0])))
    # not refused for their own sake: the NULL context is all that is left to object to
    refused("NULL context", lambda c: (setattr(c.streams[0], "log_size", 0), setattr(c.streams[0], "linear", 1)))
    refused("NULL context", lambda c: (setattr(c.streams[0], "d_prev", None), setattr(c.streams[0], "d_ordinal", None), setattr(c.streams[0], "d_payload", None)))
    refused("NULL context", lambda c: (setattr(c.streams[1], "n_records", 0), setattr(c.streams[1], "log_size", 99)))        # no record; log_size of a block stream is not read
    refused("NULL context", lambda c: (setattr(c.streams[1], "span", 256), setattr(c.streams[1], "delta", None)))
    refused("NULL context", lambda c: (setattr(c.streams[0], "span", 0), setattr(c.streams[0], "n_records", 7)))             # span of a column stream is not read
    refused("NULL context", lambda c: setattr(c.streams[0], "delta", c.words([0, 0xFFFFFFFF, 5])))
    refused("NULL context", init=False, summary=False)
    assert lib.nx_trace_access_chain(None, None, 0, 0, None, 0, None, None, None) == NX_ERR_ARG


def test_kernels_in_lock_step_on_the_host_under_sanitizers(tmp_path):
    """csrc/access_chain.hip with csrc/access_history.cuh as host C++ (tests/native/prev_emul/internal.h: 256 lock-step fibers per block, waves of 64): GIVEN-only
    calls, one key chained 1 .. 3000 times with a GIVEN at the start, the middle and the end, column and block streams mixed at every
    span and record count with random rules, bytes, flags, NULL columns, epochs, misplaced buffers and short summaries, an absorb loop,
    keys up to 2^32 - 1 and every refusal of the device against a walk over a map, with ASan and UBSan watching every LDS, histogram,
    placement, aggregate and summary index, guard words behind every output — and the device-memory bound of the header.  Twice: as
    built, and with a block cap of 2, where a block of the sort takes more tiles than the minimum."""
    gxx = shutil.which("g++")
    native = os.path.join(ROOT, "tests", "native")
    csrc = os.path.join(ROOT, "nexus-zkvm_amd", "csrc")
    shutil.copy(os.path.join(csrc, "access_chain.hip"), str(tmp_path / "access_chain_emu.cpp"))
    shutil.copy(os.path.join(csrc, "trace_rows.h"), str(tmp_path / "trace_rows.h"))
    shutil.copy(os.path.join(csrc, "count_pass.cuh"), str(tmp_path / "count_pass.cuh"))
    shutil.copy(os.path.join(csrc, "access_history.cuh"), str(tmp_path / "access_history.cuh"))
    shutil.copy(os.path.join(native, "prev_emul", "internal.h"), str(tmp_path / "internal.h"))
    for cap, flags in ((1024, []), (2, ["-DNX_COUNT_PASS_MAX_BLOCKS=2"])):
        exe = str(tmp_path / ("access_chain_emul_%d" % cap))
        subprocess.run([gxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-Wno-unknown-pragmas"] + flags +
                       ["-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"), os.path.join(native, "access_chain_emul.cpp"), "-o", exe], check=True, capture_output=True)
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "\n0 failures" in r.stdout and r.stdout.count(" OK ") >= 130 and "FAIL" not in r.stdout and ("block cap %d\n" % cap) in r.stdout
        assert "2^11 rows and two records of 4 " in r.stdout and "PLAN NOT REACHED" not in r.stdout
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def _mixed(rng, rules=True):
    key_bits, npay = [8, 5], 3
    streams = []
    for log, epoch, linear, flags in ((7, 0, True, False), (9, 1, False, True), (9, 1, False, False), (6, 1, False, True), (0, 1, True, False), (3, 7, False, False)):
        rule = [M.ADD if rules and rng.integers(0, 2) else M.GIVEN for _ in range(npay)]
        streams.append(M.column_stream(rng, key_bits, log, npay, rng.integers(0, 1 << 10, 1 << log), rule=rule, delta=[1, 0, 0xFFFFFFFF], flags=flags, null_payload=(1,),
                                       epoch=epoch, linear=linear))
    if rules:
        streams.insert(2, M.block_stream(rng, key_bits, [0, 1, 7, 300, 511, 600], 200, npay, rng.integers(0, 1 << 10, 6), rule=[M.ADD, M.GIVEN | M.BYTES, M.GIVEN], flags=True, epoch=1))
        streams.append(M.block_stream(rng, key_bits, [3, 511], 7, npay, [5, 1000], rule=None, delta=None, epoch=1))
        streams.append(M.block_stream(rng, key_bits, [], 4, npay, [], epoch=1))
    return streams, key_bits, npay


def test_the_model_by_sorting_is_the_sequential_model():
    """the twin that judges the larger device cases, against the walk: column streams alone with every rule GIVEN (the shape the
    compatibility cases have), then epochs, mixed sizes, block streams beside column streams on shared rows, random rules, flags, NULL
    columns, an empty block stream — and every kind of refused input"""
    streams, key_bits, npay = _mixed(np.random.default_rng(2031), rules=False)
    M.same_answers(M.model_by_sorting(streams, key_bits, npay, [1, 2, 3]), M.model(streams, key_bits, npay, [1, 2, 3]))
    for seed in (2032, 2033):
        streams, key_bits, npay = _mixed(np.random.default_rng(seed))
        want = M.model(streams, key_bits, npay, [P - 1, 0, 77])
        assert want["bad"] is None
        M.same_answers(M.model_by_sorting(streams, key_bits, npay, [P - 1, 0, 77]), want)
        M.same_answers(M.model_by_sorting(streams, key_bits, npay), M.model(streams, key_bits, npay))
    streams[2]["key"][0][4], streams[2]["key"][1][4], streams[2]["flag"][4] = 100, 31, 1      # 31 * 256 + 100 = 8036 reaches 2^13 at sub-access 156
    want = M.model(streams, key_bits, npay)
    assert want["bad"] == (2, 4, 156, M.BAD_SUB)
    M.same_answers(M.model_by_sorting(streams, key_bits, npay), want)
    streams[2]["key"][1][1], streams[2]["flag"][1] = 32, 2
    assert M.model(streams, key_bits, npay)["bad"] == (2, 1, 0, M.BAD_ENTRY) == M.model_by_sorting(streams, key_bits, npay)["bad"]
    streams[1]["key"][0][9], streams[1]["flag"][9] = 256, 1
    assert M.model(streams, key_bits, npay)["bad"] == (1, 9, 0, M.BAD_ENTRY) == M.model_by_sorting(streams, key_bits, npay)["bad"]
    streams[1]["flag"][9], streams[2]["flag"][1], streams[2]["flag"][4] = 0, 0, 0
    streams[2]["row"] = np.array([0, 1, 7, 7, 511, 600], np.uint32)
    assert M.model(streams, key_bits, npay)["bad"] == (2, 3, 0, M.BAD_ORDER) == M.model_by_sorting(streams, key_bits, npay)["bad"]


def test_the_walk_reproduces_the_history_written_out_by_hand():
    """tests/golden/access_chain_history.json: an image, a store, a load, two block records on one buffer, a load after them, a record on
    a second buffer that overlaps the first by 8 bytes, a load of a byte only that one wrote — every previous timestamp, previous value
    and ordinal and the final state derived by hand from update_state_timestamps and last_access.insert"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "access_chain_history.json")))
    from prev_access_model import to_storage
    im, mem, kec = g["image"], g["mem"], g["keccak"]
    log = mem["log_size"]
    col = lambda a: to_storage(np.array(a, np.uint32), log)
    assert mem["ts"] == [r + 1 for r in range(1 << log)]
    streams = [{"key": [np.array(im["address"], np.uint32)], "flag": None, "payload": [None, np.array(im["value"], np.uint32)], "log_size": im["log_size"], "epoch": 0, "linear": True},
               {"key": [col(mem["address"])], "flag": col(mem["accessed"]), "payload": [col(mem["ts"]), col(mem["value"])], "log_size": log, "epoch": 1},
               {"row": np.array(kec["row"], np.uint32), "span": kec["span"], "key": [np.array(kec["address"], np.uint32)], "flag": None,
                "payload": [None, np.array(kec["out"], np.uint32).reshape(-1)], "rule": [M.ADD, M.GIVEN | M.BYTES], "delta": [1, 0], "epoch": 1}]
    for r in (M.model(streams, g["key_bits"], 2, g["init"]), M.model_by_sorting(streams, g["key_bits"], 2, g["init"])):
        assert r["bad"] is None
        assert np.array_equal(r["prev"][1][0], col(mem["ts_prev"])) and np.array_equal(r["prev"][1][1], col(mem["val_prev"])) and np.array_equal(r["ordinal"][1], col(mem["ordinal"]))
        flat = lambda a: np.array(a, np.uint32).reshape(-1)
        assert np.array_equal(r["prev"][2][0], flat(kec["ts_prev"])) and np.array_equal(r["prev"][2][1], flat(kec["val_prev"])) and np.array_equal(r["ordinal"][2], flat(kec["ordinal"]))
        assert np.array_equal(r["left"][2][0], flat(kec["ts_prev"]) + 1) and np.array_equal(r["left"][2][1], flat(kec["out"]))
        f = g["final"]
        assert (r["keys"].tolist(), r["counts"].tolist(), r["last"][0].tolist(), r["last"][1].tolist()) == (f["address"], f["accesses"], f["ts"], f["value"])
