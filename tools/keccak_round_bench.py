"""nx_trace_keccak_round at the size of BASELINE config #5's keccak precompile: 2^14 instances through both KeccakRound components,
  first   16 rounds from round 0, 2^18 rows
  second   8 rounds from round 16, 2^17 rows
1705 main columns each (the 9 preprocessed columns are not written: they are committed once per statement shape), next to the two
yardsticks of the project: nx_copy of as many column words as the call stores (the store-bandwidth yardstick: the copy reads and
writes that many words) and nx_upload_columns_narrow of the 1705 produced columns as NX_COL_U8 — what a host that had computed them
pays on PCIe today.  One context; HIP-event time on the context's stream around each call, medians of warmed rounds that alternate
between the three in one process.
  timeout -k 10 900 python tools/keccak_round_bench.py [log_instances=14] [rounds=5] [output.json]
Every step runs under a deadline of its own: a step that exceeds it ends the process (exit status 124) before anything else is
started on the GPU.  Writes profiles/keccak_round_bench.json (or the named file) and prints the same line."""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "keccak_round_bench.json")
n_inst = 1 << log_inst
MAIN = nz.KECCAK_ROUND_MAIN_COLS


class step:
    """`with step(name, seconds):` — the deadline of one step."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def expired():
            sys.stderr.write(f"keccak_round_bench: step '{self.name}' exceeded {self.seconds} s\n")
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


rng = np.random.default_rng(68)
out = {"tool": "keccak_round_bench", "instances": n_inst, "rounds": rounds, "main_columns": MAIN, "components": {}}
with step("states", 120):
    words = np.ascontiguousarray(rng.integers(0, 1 << 64, size=(n_inst, 25), dtype=np.uint64), "<u8").view(np.uint32).reshape(-1)
    log_words = int(len(words) - 1).bit_length()
    d_states = be.columns_from_host(np.concatenate([words, np.zeros((1 << log_words) - len(words), np.uint32)]))
    d_out = be.columns(1, log_words)
for name, first, log_rounds in (("first", 0, 4), ("second", 16, 3)):
    log = log_inst + log_rounds
    n = 1 << log
    with step("fill " + name, 240):
        main = be.columns(MAIN, log)
        src, dst = be.columns(MAIN, log), be.columns(MAIN, log)
        produced = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(MAIN)]     # byte limbs, as the columns of this trace are
        ptrs = list(main.col_ptrs())
        be.sync()
    with step("run " + name, 420):
        call = lambda: be.trace_keccak_round(d_states.ptr.value, n_inst, first, log_rounds, log, ptrs, None, d_out.ptr.value)
        copy = lambda: be._chk(be.L.nx_copy(be.ctx, dst.ptr, src.ptr, C.c_size_t(MAIN * n)))
        up = lambda: be.upload_columns_narrow(produced, coset_order=True).free()
        ms = {"keccak_round": [], "nx_copy": [], "narrow_upload": []}
        for r in range(rounds + 1):
            for key, f in (("keccak_round", call), ("nx_copy", copy), ("narrow_upload", up)):
                t = once(f)
                if r:
                    ms[key].append(t)
        res = {key: stats(v) for key, v in ms.items()}
        kr = res["keccak_round"]["median_ms"]
        res.update({"first_round": first, "rounds_per_instance": 1 << log_rounds, "log_size": log, "words_stored": MAIN * n,
                    "stored_gb_per_s": round(MAIN * n * 4 / kr / 1e6, 1), "copy_written_gb_per_s": round(MAIN * n * 4 / res["nx_copy"]["median_ms"] / 1e6, 1),
                    "upload_host_gb_per_s": round(MAIN * n / res["narrow_upload"]["median_ms"] / 1e6, 1),
                    "ratio_to_nx_copy": round(kr / res["nx_copy"]["median_ms"], 3), "ratio_to_narrow_upload": round(kr / res["narrow_upload"]["median_ms"], 4)})
        out["components"][name] = res
    del main, src, dst, produced
be.close()
line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
print(line)
