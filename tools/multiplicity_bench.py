"""nx_logup_multiplicities at the v1 main trace's shape: 340 byte-limb columns of 2^22 rows looked up in a 256-row range table, for
three value distributions — uniform bytes, all-zero columns, 90 % zeros — next to nx_copy of the same 340 columns, the yardstick for
reading those bytes (it also writes them).  One context; every figure is HIP-event time on the context's stream around the whole
blocking call (descriptor upload, count, scatter, residual, read-back).
  timeout -k 10 600 python tools/multiplicity_bench.py [log=22] [columns=340] [rounds=5]
Every step runs under a deadline of its own: a step that exceeds it ends the process (exit status 124) before anything else is
started on the GPU.  Writes profiles/multiplicity_bench.json and prints the same line."""
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

log = int(sys.argv[1]) if len(sys.argv) > 1 else 22
n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 340
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
P = (1 << 31) - 1
n = 1 << log
N_SRC = 4            # distinct columns per distribution; the slab's columns are copies of them (a histogram's time does not see that)


class step:
    """`with step(name, seconds):` — the deadline of one step."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def expired():
            sys.stderr.write(f"multiplicity_bench: step '{self.name}' exceeded {self.seconds} s\n")
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
    # the HIP runtime the library itself runs on (already mapped), for the events
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
    slab, dst = be.columns(n_cols, log), be.columns(n_cols, log)
    src = be.columns(N_SRC, log)
    table = be.columns_from_host(np.arange(256, dtype=np.uint32))
    mult = be.columns(1, 8)
col = lambda k: slab.ptr.value + k * (4 << log)
uses = [([col(k)], None, log) for k in range(n_cols)]


def timed(call):
    """HIP-event milliseconds of `rounds` runs after one warm-up."""
    ms = []
    for r in range(rounds + 1):
        hip_chk(hip.hipEventRecord(ev0, stream))
        call()
        hip_chk(hip.hipEventRecord(ev1, stream))
        hip_chk(hip.hipEventSynchronize(ev1))
        t = C.c_float()
        hip_chk(hip.hipEventElapsedTime(C.byref(t), ev0, ev1))
        if r:
            ms.append(t.value)
    return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3)}


rng = np.random.default_rng(22)
dists = {"uniform_bytes": lambda: rng.integers(0, 256, (N_SRC, n), dtype=np.uint32),
         "all_zero": lambda: np.zeros((N_SRC, n), np.uint32),
         "zeros_90_percent": lambda: np.where(rng.random((N_SRC, n)) < 0.9, 0, rng.integers(0, 256, (N_SRC, n))).astype(np.uint32)}
bytes_read = 4 * n_cols * n
out = {"tool": "multiplicity_bench", "log_size": log, "columns": n_cols, "table_rows": 256, "rounds": rounds, "looked_up_values": n_cols * n, "bytes_read": bytes_read,
       "multiplicities": {}}
for name, make in dists.items():
    with step("fill " + name, 120):
        host = make()
        src.upload(host)
        for k in range(n_cols):
            be._chk(be.L.nx_copy(be.ctx, C.c_void_p(col(k)), C.c_void_p(src.ptr.value + (k % N_SRC) * (4 << log)), C.c_size_t(n)))
        be.sync()
    with step("count " + name, 120):
        res = timed(lambda: be.logup_multiplicities(uses, [table.ptr.value], 8, [8], mult.ptr.value))
        got = mult.to_cpu().reshape(-1).astype(object)
        want = sum(np.bincount(host[j], minlength=256).astype(object) * len(range(j, n_cols, N_SRC)) for j in range(N_SRC)) % P
        res["GBs_read"] = round(bytes_read / res["median_ms"] / 1e6, 1)
        res["equals_numpy"] = bool((got == want).all())
        out["multiplicities"][name] = res
with step("nx_copy", 120):
    res = timed(lambda: be._chk(be.L.nx_copy(be.ctx, dst.ptr, slab.ptr, C.c_size_t(n_cols * n))))
    res["GBs_read"] = round(bytes_read / res["median_ms"] / 1e6, 1)
    out["nx_copy_same_columns"] = res
for name, r in out["multiplicities"].items():
    r["fraction_of_copy_read_rate"] = round(res["median_ms"] / r["median_ms"], 3)
u, z = out["multiplicities"]["uniform_bytes"]["median_ms"], out["multiplicities"]["all_zero"]["median_ms"]
out["all_zero_over_uniform"] = round(z / u, 3)
be.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "multiplicity_bench.json"), "w") as f:
    f.write(line + "\n")
print(line)
