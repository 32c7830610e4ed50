"""nx_trace_partition_create / nx_trace_partition_fill at the size of a v2 execution: 2^22 steps, 8 source columns, 40 classes, each
class a destination of 20 limb columns and IsLocalPad, in two distributions — uniform, and one class holding half the steps with ten
classes absent — next to the two yardsticks of the project: nx_copy of as many words as the fill stores (the store-bandwidth
yardstick: the copy reads and writes that many words) and nx_upload_columns_narrow of the produced columns from host memory (NX_COL_U8
for limbs of up to 8 bits and the padding flag, NX_COL_U16 for the others), which is what a host that had built them pays today.  One
context; HIP-event time on the context's stream around each call, medians of warmed rounds that alternate between the four in one
process.  create is blocking, so its time includes the copy of the counts to the host; the fill's descriptor tables are built by the
library inside the timed call, as every caller pays them.
  timeout -k 10 900 python tools/trace_partition_bench.py [log_steps=22] [rounds=5] [output.json]
Every step runs under a deadline of its own: a step that exceeds it ends the process (exit status 124) before anything else is
started on the GPU.  Writes profiles/trace_partition_bench.json (or the named file) and prints the same line."""
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

log_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 22
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "trace_partition_bench.json")
n_steps, N_SRC, N_CLASSES, MIN_LOG = 1 << log_steps, 8, 40, 4
# 20 limb columns over the 8 sources: pc and clk as half-words, three operand words as bytes, a half-word pair, a byte and a 5-bit field
LIMBS = [(0, 0, 16), (0, 16, 16), (1, 0, 16), (1, 16, 16)] + [(s, 8 * j, 8) for s in (2, 3, 4) for j in range(4)] + [(5, 0, 16), (5, 16, 16), (6, 0, 8), (7, 7, 5)]
assert len(LIMBS) == 20


class step:
    """`with step(name, seconds):` — the deadline of one step."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def expired():
            sys.stderr.write(f"trace_partition_bench: step '{self.name}' exceeded {self.seconds} s\n")
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


def class_column(rng, dist):
    if dist == "uniform":
        return rng.integers(0, N_CLASSES, n_steps, dtype=np.uint32)
    # one class holds half the steps, ten classes are absent, the other 29 share the rest; runs of one opcode as an execution has them
    present = np.array([c for c in range(1, N_CLASSES) if c % 4 != 1], np.uint32)[:29]
    cls = present[rng.integers(0, len(present), n_steps)]
    cls[rng.random(n_steps) < 0.5] = 0
    return cls


rng = np.random.default_rng(71)
out = {"tool": "trace_partition_bench", "steps": n_steps, "rounds": rounds, "source_columns": N_SRC, "classes": N_CLASSES, "limb_columns_per_class": len(LIMBS), "shapes": {}}
with step("sources", 120):
    d_src = [be.columns_from_host(rng.integers(0, 1 << 32, n_steps, dtype=np.uint64).astype(np.uint32)) for _ in range(N_SRC)]
    src_ptrs = [d.ptr.value for d in d_src]
for dist in ("uniform", "half_in_one_class"):
    with step(dist + ": inputs", 240):
        cls = class_column(rng, dist)
        d_cls = be.columns_from_host(cls)
        counts, part = be.trace_partition(d_cls.ptr.value, n_steps, N_CLASSES)
        assert np.array_equal(counts, np.bincount(cls, minlength=N_CLASSES))
        logs = [nz.partition_log_size(int(c), MIN_LOG) for c in counts]
        slabs = [be.columns(len(LIMBS) + 1, lg) for lg in logs]
        dests = []
        for c, (lg, slab) in enumerate(zip(logs, slabs)):
            ptrs = list(slab.col_ptrs())
            dests.append({"cls": c, "log_size": lg, "cols": ptrs[:len(LIMBS)], "limbs": LIMBS, "is_pad": ptrs[len(LIMBS)]})
        stored = sum((len(LIMBS) + 1) << lg for lg in logs)
        log_copy = int(stored - 1).bit_length()
        src, dst = be.columns(1, log_copy), be.columns(1, log_copy)
        narrow = [np.uint8 if bits <= 8 else np.uint16 for _, _, bits in LIMBS] + [np.uint8]
        produced = [[rng.integers(0, 2, 1 << lg, dtype=t) for t in narrow] for lg in logs]
        part.destroy()
        be.sync()
    with step(dist + ": run", 420):
        parts = []

        def create():
            parts.append(be.trace_partition(d_cls.ptr.value, n_steps, N_CLASSES)[1])

        def fill():
            parts[-1].fill(src_ptrs, dests)

        def copy():
            be._chk(be.L.nx_copy(be.ctx, dst.ptr, src.ptr, C.c_size_t(stored)))

        def upload():
            for cols in produced:
                be.upload_columns_narrow(cols, coset_order=True).free()

        ms = {"create": [], "fill": [], "nx_copy": [], "narrow_upload": []}
        for r in range(rounds + 1):
            for key, f in (("create", create), ("fill", fill), ("nx_copy", copy), ("narrow_upload", upload)):
                t = once(f)
                if r:
                    ms[key].append(t)
            parts.pop().destroy()
        res = {key: stats(v) for key, v in ms.items()}
        fl, cr = res["fill"]["median_ms"], res["create"]["median_ms"]
        host_bytes = sum(c.nbytes for cols in produced for c in cols)
        res.update({"counts_max": int(counts.max()), "classes_absent": int((counts == 0).sum()), "log_sizes": sorted(set(logs)), "words_stored": stored,
                    "table_bytes": 4 * n_steps * (N_SRC + 1), "upload_host_bytes": host_bytes, "stored_gb_per_s": round(stored * 4 / fl / 1e6, 1),
                    "copy_written_gb_per_s": round(stored * 4 / res["nx_copy"]["median_ms"] / 1e6, 1),
                    "fill_ratio_to_nx_copy": round(fl / res["nx_copy"]["median_ms"], 3), "fill_ratio_to_narrow_upload": round(fl / res["narrow_upload"]["median_ms"], 4),
                    "create_plus_fill_ratio_to_narrow_upload": round((cr + fl) / res["narrow_upload"]["median_ms"], 4)})
        out["shapes"][dist] = res
    with step(dist + ": release", 60):
        for s in slabs + [src, dst, d_cls]:
            s.free()
be.close()
line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
print(line)
