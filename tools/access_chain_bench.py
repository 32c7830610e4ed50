"""nx_trace_access_chain at the shape of the RAM of a keccak guest: the 4 byte streams of the load/store chip, 2^22 rows each (epoch
1, the 32-bit address as 4 byte limbs, payload (timestamp = row + 1, value), flags), a linear image of 2^16 rows in epoch 0 and one
block stream of 2^14 keccak records of span 200 (timestamp ADD 1, value GIVEN | BYTES) on ascending rows of the trace — next to two
yardsticks:
  prev_access    nx_trace_prev_access on the column streams alone, same buffers: the parent capability, what chaining and the block
                 stream cost on top of it;
  narrow_upload  nx_upload_columns_narrow of the columns the call produces (per byte stream the previous timestamp as u32 and the
                 previous value as u8; the block stream's two outputs, 2^14 x 200 words each, counted as one u32 and one u8 column of
                 2^22 rows, 28 % more than they are) — what a host that had walked the history would pay on PCIe alone.
One context; HIP-event time on the context's stream around each whole blocking call, medians of warmed rounds that alternate between
the three in one process.
  timeout -k 10 900 python tools/access_chain_bench.py [log=22] [log_records=14] [rounds=5]
Every step runs under a deadline of its own: a step that exceeds it ends the process (exit status 124) before anything else is
started on the GPU.  Writes profiles/access_chain_bench.json and prints the same line."""
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
log_rec = int(sys.argv[2]) if len(sys.argv) > 2 else 14
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
n, n_rec, SPAN = 1 << log, 1 << log_rec, 200
LOG_IMAGE = min(16, log)
KEY_BITS, NPAY = [8, 8, 8, 8], 2


class step:
    """`with step(name, seconds):` — the deadline of one step."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def expired():
            sys.stderr.write(f"access_chain_bench: step '{self.name}' exceeded {self.seconds} s\n")
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


def limbs(a):
    return [((a >> np.uint64(8 * i)) & np.uint64(255)).astype(np.uint32) for i in range(4)]


def words_on_device(words):
    """any number of words in a slab of whole columns"""
    lg = max(1, int(len(words) - 1).bit_length())
    buf = np.zeros(1 << lg, np.uint32)
    buf[:len(words)] = words
    return be.columns_from_host(buf)


rng = np.random.default_rng(41)
out = {"tool": "access_chain_bench", "log_size": log, "records": n_rec, "span": SPAN, "rounds": rounds}
with step("fill", 300):
    keep, cols = [], []
    m = 1 << LOG_IMAGE
    d = be.columns_from_host(np.stack(limbs(0x10000 + np.arange(m, dtype=np.uint64)) + [rng.integers(0, 256, m, dtype=np.uint32)]))
    keep.append(d)
    cols.append({"key": [d.ptr.value + i * (4 << LOG_IMAGE) for i in range(4)], "payload": [None, d.ptr.value + 4 * (4 << LOG_IMAGE)], "log_size": LOG_IMAGE, "epoch": 0, "linear": True})
    HEAP, HEAP_BYTES = 0x800000, 1 << 20
    pos = np.arange(n, dtype=np.uint64)
    # natural coset row of every storage position, vectorised: bit-reverse, then even rows first, odd rows backwards
    rev = np.zeros(n, np.uint64)
    for b in range(log):
        rev |= ((pos >> np.uint64(b)) & np.uint64(1)) << np.uint64(log - 1 - b)
    nat = np.where(rev < n // 2, 2 * rev, 2 * (n - 1 - rev) + 1)
    ts = (nat + 1).astype(np.uint32)
    for s in range(4):                                                 # half the touches inside the image, half in the heap the records hash
        a = np.where(rng.random(n) < 0.5, 0x10000 + rng.integers(0, m, n), HEAP + rng.integers(0, HEAP_BYTES, n)).astype(np.uint64)
        d = be.columns_from_host(np.stack(limbs(a) + [(rng.random(n) < 0.8).astype(np.uint32), ts, rng.integers(0, 256, n, dtype=np.uint32)]))
        o = be.columns(NPAY, log)
        keep += [d, o]
        col = lambda i, d=d: d.ptr.value + i * (4 << log)
        cols.append({"key": [col(i) for i in range(4)], "flag": col(4), "payload": [col(5), col(6)], "prev": [o.ptr.value + c * (4 << log) for c in range(NPAY)], "log_size": log, "epoch": 1})
    rows = np.sort(rng.choice(n, n_rec, replace=False)).astype(np.uint32)
    addr = (HEAP + rng.integers(0, HEAP_BYTES - SPAN, n_rec)).astype(np.uint64)
    d_row, d_key = words_on_device(rows), [words_on_device(k) for k in limbs(addr)]
    d_bytes = words_on_device(rng.integers(0, 1 << 32, n_rec * SPAN // 4, dtype=np.uint32))
    d_out = [words_on_device(np.zeros(n_rec * SPAN, np.uint32)) for _ in range(NPAY)]
    keep += [d_row, d_bytes] + d_key + d_out
    block = {"key": [k.ptr.value for k in d_key], "row": d_row.ptr.value, "n_records": n_rec, "span": SPAN, "payload": [None, d_bytes.ptr.value],
             "rule": [nz.CHAIN_ADD, nz.CHAIN_GIVEN | nz.CHAIN_BYTES], "delta": [1, 0], "prev": [x.ptr.value for x in d_out], "epoch": 1}
    produced = [rng.integers(0, 1 << 32, n, dtype=np.uint32) for _ in range(5)] + [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(5)]
    be.sync()
with step("run", 600):
    chain = lambda: be.trace_access_chain(cols + [block], KEY_BITS, NPAY)
    prev = lambda: be.trace_prev_access(cols, KEY_BITS, NPAY)
    up = lambda: be.upload_columns_narrow(produced, coset_order=True).free()
    n_keys, n_keys_prev = chain(), prev()
    ms = {"access_chain": [], "prev_access": [], "narrow_upload": []}
    for r in range(rounds + 1):
        for name, f in (("access_chain", chain), ("prev_access", prev), ("narrow_upload", up)):
            t = once(f)
            if r:
                ms[name].append(t)
    out.update({name: stats(v) for name, v in ms.items()})
    ac = out["access_chain"]["median_ms"]
    elems, elems_prev = m + 4 * n + n_rec * SPAN, m + 4 * n
    out.update({"elements": elems, "elements_of_the_column_streams": elems_prev, "distinct_keys": int(n_keys), "distinct_keys_of_the_column_streams": int(n_keys_prev),
                "ratio_to_prev_access": round(ac / out["prev_access"]["median_ms"], 3), "ratio_to_narrow_upload": round(ac / out["narrow_upload"]["median_ms"], 3),
                "ns_per_element": round(ac * 1e6 / elems, 3), "prev_access_ns_per_element": round(out["prev_access"]["median_ms"] * 1e6 / elems_prev, 3),
                "accesses_per_us": round(elems / ac / 1e3, 1)})
del keep
be.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "access_chain_bench.json"), "w") as f:
    f.write(line + "\n")
print(line)
