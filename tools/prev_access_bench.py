"""nx_trace_prev_access at the two shapes of the reference's memory checking, 2^22 rows:
  registers  3 streams of one epoch, a 5-bit key, 8 payload limbs (4 timestamp + 4 value bytes), flags on every stream;
  ram        4 byte streams of epoch 1, the 32-bit address as 4 byte limbs, 5 payload limbs (4 timestamp bytes + the value byte),
             flags on every stream, plus a linear image of 2^16 rows in epoch 0
next to the two yardsticks of the project: nx_copy of as many words as the call reads plus writes (the traffic floor of its inputs and
outputs; the sort's own traffic comes on top) and nx_upload_columns_narrow of the produced columns as NX_COL_U8 — what a host that
had computed them would pay on PCIe alone, and what the call replaces.  One context; HIP-event time on the context's stream around
each whole blocking call, medians of warmed rounds that alternate between the three in one process.
  timeout -k 10 900 python tools/prev_access_bench.py [log=22] [rounds=5]
Every step runs under a deadline of its own: a step that exceeds it ends the process (exit status 124) before anything else is
started on the GPU.  Writes profiles/prev_access_bench.json and prints the same line."""
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
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
P = (1 << 31) - 1
n = 1 << log
LOG_IMAGE = min(16, log)


class step:
    """`with step(name, seconds):` — the deadline of one step."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def expired():
            sys.stderr.write(f"prev_access_bench: step '{self.name}' exceeded {self.seconds} s\n")
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


rng = np.random.default_rng(31)


def build(shape):
    """-> (the call, words read + written, host copies of the produced columns as bytes, radix passes, rows in all)"""
    if shape == "registers":
        n_streams, key_bits, npay, image = 3, [5], 8, None
    else:
        n_streams, key_bits, npay, image = 4, [8, 8, 8, 8], 5, LOG_IMAGE
    k = len(key_bits)
    keep, streams, words = [], [], 0
    if image is not None:
        m = 1 << image
        addr = (0x10000 + np.arange(m, dtype=np.uint64)).astype(np.uint64)
        d = be.columns_from_host(np.stack([((addr >> np.uint64(8 * i)) & np.uint64(255)).astype(np.uint32) for i in range(4)] + [rng.integers(0, 256, m, dtype=np.uint32)]))
        keep.append(d)
        col = lambda i, d=d, lg=image: d.ptr.value + i * (4 << lg)
        streams.append({"key": [col(i) for i in range(4)], "payload": [None] * 4 + [col(4)], "log_size": image, "epoch": 0, "linear": True})
        words += 5 * m
    for s in range(n_streams):
        if shape == "registers":
            keys = [rng.integers(0, 32, n, dtype=np.uint32)]
        else:                                                          # three quarters of the touches inside the image, the rest in a 2^20-byte heap
            a = np.where(rng.random(n) < 0.75, 0x10000 + rng.integers(0, 1 << LOG_IMAGE, n), 0x800000 + rng.integers(0, 1 << 20, n)).astype(np.uint64)
            keys = [((a >> np.uint64(8 * i)) & np.uint64(255)).astype(np.uint32) for i in range(4)]
        flag = (rng.random(n) < 0.8).astype(np.uint32)
        pay = [rng.integers(0, 256, n, dtype=np.uint32) for _ in range(npay)]
        d = be.columns_from_host(np.stack(keys + [flag] + pay))
        o = be.columns(npay, log)
        keep += [d, o]
        col = lambda i, d=d: d.ptr.value + i * (4 << log)
        streams.append({"key": [col(i) for i in range(k)], "flag": col(k), "payload": [col(k + 1 + c) for c in range(npay)],
                        "prev": [o.ptr.value + c * (4 << log) for c in range(npay)], "log_size": log, "epoch": 1})
        words += (k + 1 + 2 * npay) * n
    rows = sum(1 << s["log_size"] for s in streams)
    produced = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(n_streams * npay)]   # byte limbs, as the prev columns of a byte-limb trace are
    passes = sum(key_bits) // 8 + 1
    return (lambda: be.trace_prev_access(streams, key_bits, npay)), words, produced, passes, rows, keep


out = {"tool": "prev_access_bench", "log_size": log, "rounds": rounds, "shapes": {}}
for shape in ("registers", "ram"):
    with step("fill " + shape, 240):
        call, words, produced, passes, rows, keep = build(shape)
        half_log = int(np.ceil(np.log2(words // 2)))
        src, dst = be.columns(1, half_log), be.columns(1, half_log)
        be.sync()
    with step("run " + shape, 420):
        copy = lambda: be._chk(be.L.nx_copy(be.ctx, dst.ptr, src.ptr, C.c_size_t(words // 2)))    # words / 2 read + words / 2 written
        up = lambda: be.upload_columns_narrow(produced, coset_order=True).free()
        n_keys = call()
        ms = {"prev_access": [], "nx_copy": [], "narrow_upload": []}
        for r in range(rounds + 1):
            for name, f in (("prev_access", call), ("nx_copy", copy), ("narrow_upload", up)):
                t = once(f)
                if r:
                    ms[name].append(t)
        res = {name: stats(v) for name, v in ms.items()}
        pa = res["prev_access"]["median_ms"]
        res.update({"rows_in_all": rows, "distinct_keys": int(n_keys), "radix_passes": passes, "words_read_plus_written": words, "produced_columns": len(produced),
                    "ratio_to_nx_copy": round(pa / res["nx_copy"]["median_ms"], 2), "ratio_to_narrow_upload": round(pa / res["narrow_upload"]["median_ms"], 3),
                    "accesses_per_us": round(rows / pa / 1e3, 1)})
        out["shapes"][shape] = res
    del keep, src, dst
be.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "prev_access_bench.json"), "w") as f:
    f.write(line + "\n")
print(line)
