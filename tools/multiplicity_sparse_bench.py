"""nx_logup_multiplicities_sparse at the shape of a RAM boundary: uses of 2^22 rows keyed by two 16-bit address limbs against
  (a) a table of 2^20 rows of random distinct 32-bit addresses (uniform), and a table of 2^20 rows whose 2^16 table rows are the keys
      of one 64 KiB page (clustered: all keys share their top 16 bits — there are only 2^16 such keys, the other rows are no table rows);
  (b) the same uses restricted to 20-bit keys ([16, 4]) against the full 2^20-row table, through nx_logup_multiplicities and through
      the sparse call: what the search costs where both apply;
  (c) nx_copy of the same use columns, the yardstick for reading those bytes (it also writes them).
One context; every figure is HIP-event time on the context's stream around the whole blocking call (descriptor upload, sort of the
table, count, scatter, read-back); the cases alternate inside every round, the median of the warmed rounds is reported.
  timeout -k 10 600 python tools/multiplicity_sparse_bench.py [log_use=22] [log_table=20] [rounds=5] [lib=PATH] [out=NAME]
lib: another build of the library (e.g. one compiled with -DNX_MULT_SPARSE_LDS_LOG_KEYS=1, two splitters: a plain binary search in
global memory) measured by the same tool; out: the file name under profiles/.  Every step runs under a deadline of its own: a step
that exceeds it ends the process (exit status 124) before anything else is started on the GPU.  Writes
profiles/multiplicity_sparse_bench.json and prints the same line."""
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

pos = [a for a in sys.argv[1:] if "=" not in a]
opt = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
log_use = int(pos[0]) if len(pos) > 0 else 22
log_table = int(pos[1]) if len(pos) > 1 else 20
rounds = int(pos[2]) if len(pos) > 2 else 5
if "lib" in opt:
    nz.LIB_PATH = os.path.abspath(opt["lib"])
P = (1 << 31) - 1
n, nt = 1 << log_use, 1 << log_table
assert 16 <= log_table <= 20


class step:
    """`with step(name, seconds):` — the deadline of one step."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def expired():
            sys.stderr.write(f"multiplicity_sparse_bench: step '{self.name}' exceeded {self.seconds} s\n")
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


def once(call):
    hip_chk(hip.hipEventRecord(ev0, stream))
    call()
    hip_chk(hip.hipEventRecord(ev1, stream))
    hip_chk(hip.hipEventSynchronize(ev1))
    t = C.c_float()
    hip_chk(hip.hipEventElapsedTime(C.byref(t), ev0, ev1))
    return t.value


def limbs(keys, bits):
    out, shift = [], 0
    for b in bits:
        out.append(((keys >> np.uint64(shift)) & np.uint64((1 << b) - 1)).astype(np.uint32))
        shift += b
    return out


rng = np.random.default_rng(2220)
cases, keep = {}, []


def add_case(name, key_bits, table_keys, valid, dense):
    """table_keys: one key per table row (any order); valid: None or the flag column; uses: one use of 2^log_use rows that draws the
    valid keys uniformly"""
    live = table_keys if valid is None else table_keys[valid != 0]
    picks = live[rng.integers(0, len(live), n)]
    d_use = be.columns_from_host(np.stack(limbs(picks, key_bits)))
    d_tab = be.columns_from_host(np.stack(limbs(table_keys, key_bits) + ([valid] if valid is not None else [])))
    d_out = be.columns(1, log_table)
    keep.extend([d_use, d_tab, d_out])
    k = len(key_bits)
    up = [d_use.ptr.value + i * (4 << log_use) for i in range(k)]
    tp = [d_tab.ptr.value + i * (4 << log_table) for i in range(k + 1)]
    uses = [(up, None, log_use)]
    order = np.argsort(live, kind="stable")
    want = np.zeros(nt, np.uint64)
    rows = np.arange(nt) if valid is None else np.flatnonzero(valid)
    want[rows[order]] = np.bincount(np.searchsorted(live[order], picks), minlength=len(live))
    want = (want % np.uint64(P)).astype(np.uint32)
    if dense:
        call = lambda: be.logup_multiplicities(uses, tp[:k], log_table, key_bits, d_out.ptr.value)
    else:
        call = lambda: be.logup_multiplicities_sparse(uses, tp[:k], tp[k] if valid is not None else None, log_table, key_bits, d_out.ptr.value)
    cases[name] = {"call": call, "out": d_out, "want": want, "ms": [], "table_rows": int(len(live)), "use": d_use}


with step("inputs", 240):
    uniform = np.unique(rng.integers(0, 1 << 32, nt + (nt >> 4), dtype=np.uint64))
    uniform = rng.permutation(uniform)[:nt]
    assert len(uniform) == nt
    add_case("a_uniform_32bit", [16, 16], uniform, None, False)
    page = np.uint64(0x4A3B0000)
    clustered = np.zeros(nt, np.uint64)
    valid = np.zeros(nt, np.uint32)
    where = rng.permutation(nt)[:1 << 16]
    clustered[where] = page | rng.permutation(1 << 16).astype(np.uint64)
    valid[where] = 1
    add_case("a_clustered_one_page", [16, 16], clustered, valid, False)
    full20 = rng.permutation(nt).astype(np.uint64)
    bits_b = [16, log_table - 16]
    add_case("b_20bit_dense", bits_b, full20, None, True)
    add_case("b_20bit_sparse", bits_b, full20, None, False)
    copy_src = cases["a_uniform_32bit"]["use"]
    copy_dst = be.columns(2, log_use)
    cases["c_nx_copy_use_columns"] = {"call": lambda: be._chk(be.L.nx_copy(be.ctx, copy_dst.ptr, copy_src.ptr, C.c_size_t(2 * n))), "ms": []}
    be.sync()

with step("rounds", 300):
    for r in range(rounds + 1):                      # round 0 warms; the cases alternate inside every round
        for name, c in cases.items():
            t = once(c["call"])
            if r:
                c["ms"].append(t)

bytes_read = 4 * 2 * n
out = {"tool": "multiplicity_sparse_bench", "library": os.path.relpath(nz.LIB_PATH, ROOT), "lds_log_keys_of_the_default_build": nz.MULT_SPARSE_LDS_LOG_KEYS, "log_use": log_use, "log_table": log_table,
       "rounds": rounds, "use_bytes_read": bytes_read, "cases": {}}
with step("compare", 240):
    for name, c in cases.items():
        res = {"min_ms": round(min(c["ms"]), 3), "median_ms": round(statistics.median(c["ms"]), 3), "max_ms": round(max(c["ms"]), 3)}
        res["use_GBs_read"] = round(bytes_read / res["median_ms"] / 1e6, 1)
        if "want" in c:
            res["table_rows_valid"] = c["table_rows"]
            res["equals_numpy"] = bool(np.array_equal(c["out"].to_cpu().reshape(-1), c["want"]))
        out["cases"][name] = res
copy_ms = out["cases"]["c_nx_copy_use_columns"]["median_ms"]
for name in ("a_uniform_32bit", "a_clustered_one_page"):
    out["cases"][name]["read_rate_over_copy"] = round(copy_ms / out["cases"][name]["median_ms"], 3)
out["b_sparse_over_dense"] = round(out["cases"]["b_20bit_sparse"]["median_ms"] / out["cases"]["b_20bit_dense"]["median_ms"], 3)
be.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", opt.get("out", "multiplicity_sparse_bench.json")), "w") as f:
    f.write(line + "\n")
print(line)
