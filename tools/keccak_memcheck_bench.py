"""nx_trace_keccak_memory_check at the size of BASELINE config #5's keccak precompile: 2^14 instances, one row each, the 2001 main
columns of the PermutationMemoryCheck component (is_last is not written: it is committed once per statement shape; d_states_out is),
next to the two yardsticks of the project: nx_copy of as many words as the call stores, the 50 words per instance of d_states_out
included (the store-bandwidth yardstick: the copy reads and writes that many words) and nx_upload_columns_narrow of the 2001 produced
columns — NX_COL_U8 for the 400 state bytes, the 400 carries and is_padding, NX_COL_U16 for the 1200 limbs — what a host that had
computed them pays on PCIe today.  The call is timed as the library's: its table of 2001 pointers is built once, outside the timed
region, as a caller that fills the same columns again would hold it; keccak_memory_check_binding is the same call through
HipBackend.trace_keccak_memory_check, which builds that table from a Python list every time.  One context; HIP-event time on the
context's stream around each call, medians of warmed rounds that alternate between the four in one process.
  timeout -k 10 900 python tools/keccak_memcheck_bench.py [log_instances=14] [rounds=5] [output.json]
Every step runs under a deadline of its own: a step that exceeds it ends the process (exit status 124) before anything else is
started on the GPU.  Writes profiles/keccak_memcheck_bench.json (or the named file) and prints the same line."""
import ctypes as C
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import nexus_zkvm_amd as nz

log_inst = int(sys.argv[1]) if len(sys.argv) > 1 else 14
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "keccak_memcheck_bench.json")
n_inst = 1 << log_inst
MAIN = nz.KECCAK_MEMCHECK_MAIN_COLS


class step:
    """`with step(name, seconds):` — the deadline of one step."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def expired():
            sys.stderr.write(f"keccak_memcheck_bench: step '{self.name}' exceeded {self.seconds} s\n")
            sys.stderr.flush()
            os._exit(124)
        self.t = threading.Timer(self.seconds, expired)
        self.t.daemon = True
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()
        return False


def hip_chk(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


with step("context", 120):
    be = nz.HipBackend(0)
    hip = C.CDLL(next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64.so" in l))
    for f in (hip.hipEventCreate, hip.hipEventRecord, hip.hipEventSynchronize, hip.hipEventElapsedTime):
        f.restype = C.c_int
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    stream = C.c_void_p(be.L.nx_ctx_stream(be.ctx))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_chk(hip.hipEventCreate(C.byref(ev0)))
    hip_chk(hip.hipEventCreate(C.byref(ev1)))


def once(call):
    hip_chk(hip.hipEventRecord(ev0, stream))
    call()
    hip_chk(hip.hipEventRecord(ev1, stream))
    hip_chk(hip.hipEventSynchronize(ev1))
    t = C.c_float()
    hip_chk(hip.hipEventElapsedTime(C.byref(t), ev0, ev1))
    return t.value


def stats(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3)}


rng = np.random.default_rng(70)
log, n = log_inst, n_inst
out = {"tool": "keccak_memcheck_bench", "instances": n_inst, "rounds": rounds, "main_columns": MAIN, "log_size": log}


def on_device(words):
    """uint32 words -> a slab of one column (256-byte aligned), zeros behind them"""
    log_words = max(1, int(len(words) - 1).bit_length())
    return be.columns_from_host(np.concatenate([words, np.zeros((1 << log_words) - len(words), np.uint32)]))


with step("inputs", 120):
    d_states = on_device(np.ascontiguousarray(rng.integers(0, 1 << 64, size=(n_inst, 25), dtype=np.uint64), "<u8").view(np.uint32).reshape(-1))
    d_addr = on_device(rng.integers(0, (1 << 32) - 200, n_inst, dtype=np.uint32))
    d_ts = on_device(rng.integers(0, (1 << 32) - 1, n_inst * 200, dtype=np.uint32))
    d_out = be.columns(1, max(1, int(50 * n_inst - 1).bit_length()))
with step("fill", 240):
    main = be.columns(MAIN, log)
    stored = MAIN * n + 50 * n_inst                     # the main columns and the 25 lanes of d_states_out
    src, dst = be.columns(MAIN + 50, log), be.columns(MAIN + 50, log)      # n = n_inst: 50 more columns are d_states_out's words
    # as the columns of this trace are: bytes and flags as NX_COL_U8, 16-bit limbs as NX_COL_U16
    narrow = lambda k: np.uint16 if 400 <= k < 1600 else np.uint8
    produced = [rng.integers(0, 1 << (16 if narrow(k) is np.uint16 else 8), n, dtype=narrow(k)) for k in range(MAIN)]
    ptrs = list(main.col_ptrs())
    table = (C.c_void_p * MAIN)(*[int(x) for x in ptrs])
    be.sync()
with step("run", 420):
    call = lambda: be._chk(be.L.nx_trace_keccak_memory_check(be.ctx, d_states.ptr, d_addr.ptr, d_ts.ptr, C.c_uint32(n_inst), C.c_uint32(log), table, None, d_out.ptr))
    binding = lambda: be.trace_keccak_memory_check(d_states.ptr.value, d_addr.ptr.value, d_ts.ptr.value, n_inst, log, ptrs, None, d_out.ptr.value)
    copy = lambda: be._chk(be.L.nx_copy(be.ctx, dst.ptr, src.ptr, C.c_size_t(stored)))
    up = lambda: be.upload_columns_narrow(produced, coset_order=True).free()
    ms = {"keccak_memory_check": [], "keccak_memory_check_binding": [], "nx_copy": [], "narrow_upload": []}
    for r in range(rounds + 1):
        for key, f in (("keccak_memory_check", call), ("keccak_memory_check_binding", binding), ("nx_copy", copy), ("narrow_upload", up)):
            t = once(f)
            if r:
                ms[key].append(t)
    res = {key: stats(v) for key, v in ms.items()}
    km = res["keccak_memory_check"]["median_ms"]
    host_bytes = sum(p.nbytes for p in produced)
    res.update({"words_stored": stored, "input_bytes": 1004 * n_inst, "upload_host_bytes": host_bytes,
                "stored_gb_per_s": round(stored * 4 / km / 1e6, 1), "copy_written_gb_per_s": round(stored * 4 / res["nx_copy"]["median_ms"] / 1e6, 1),
                "upload_host_gb_per_s": round(host_bytes / res["narrow_upload"]["median_ms"] / 1e6, 1),
                "ratio_to_nx_copy": round(km / res["nx_copy"]["median_ms"], 3), "ratio_to_narrow_upload": round(km / res["narrow_upload"]["median_ms"], 4)})
    out.update(res)
be.close()
line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
print(line)
