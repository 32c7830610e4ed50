"""The RV32M chips' fill (tests/rv32m_air.py fill_program: 73 columns from ValueB, ValueC and eight opcode flags, one nx_trace_program
call with one 32-bit division and one 64-bit product per row) at 2^22 rows, the eight opcodes in equal shares, next to two yardsticks:
  nx_copy of as many words as the fill stores, and
  nx_upload_columns_narrow of the 73 columns it produces as NX_COL_U8 — what a host that derives them itself pays to send them.
The fill is timed in both kernel shapes (context option "trace.vec4").  Every figure is HIP-event time on the context's stream around
the whole call; 5 warmed rounds, the candidates alternating round by round in one process; medians (min - max).  No ratio is fixed in
advance.  The device's columns are compared with the plain-integer model of tests/rv32m_model.py on the first 4096 positions.
  timeout -k 10 900 python tools/rv32m_bench.py [log=22] [rounds=5]
Every step runs under a deadline of its own: a step that exceeds it ends the process (exit status 124) before anything else is
started on the GPU.  Writes profiles/rv32m_bench.json and prints the same line."""
import ctypes as C
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import nexus_zkvm_amd as nz
import nexus_zkvm_amd.air_program as ap
import rv32m_air as A
import rv32m_model as M

log = int(sys.argv[1]) if len(sys.argv) > 1 else 22
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = 1 << log
CHECKED = min(n, 4096)


class step:
    """`with step(name, seconds):` — the deadline of one step."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def expired():
            sys.stderr.write(f"rv32m_bench: step '{self.name}' exceeded {self.seconds} s\n")
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
    hip = C.CDLL(next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64.so" in l))      # the runtime the library runs on
    for f in (hip.hipEventCreate, hip.hipEventRecord, hip.hipEventSynchronize, hip.hipEventElapsedTime):
        f.restype = C.c_int
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    stream = C.c_void_p(be.L.nx_ctx_stream(be.ctx))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_chk(hip.hipEventCreate(C.byref(ev0)))
    hip_chk(hip.hipEventCreate(C.byref(ev1)))
    n_out = M.N_COLS - M.N_SEED
    slab, dst = be.columns(M.N_COLS, log), be.columns(n_out, log)
col = lambda d, k: d.ptr.value + k * (4 << log)

with step("seeds", 300):
    rng = np.random.default_rng(22)
    owner = np.arange(n) % 8                                   # the program is row-local: a storage position is a row
    seed = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(8)] + [(owner == k).astype(np.uint8) for k in range(8)]
    for k in range(4):                                          # a zero divisor on some rows
        seed[4 + k][::61] = 0
    arrs, kinds = nz._narrow_columns(seed)
    table = (C.c_void_p * M.N_SEED)(*[col(slab, k) for k in range(M.N_SEED)])
    be._chk(be.L.nx_upload_columns_narrow(be.ctx, *nz._host_columns(arrs, kinds), M.N_SEED, log, table, 0))
    word = lambda limbs, i: sum(int(limbs[k][i]) << (8 * k) for k in range(4))
    ops = [M.OPS[i % 8] for i in range(CHECKED)]
    _, want = M.seeds_and_trace(ops, [(word(seed[0:4], i), word(seed[4:8], i)) for i in range(CHECKED)])

prog = A.fill_program()
ptrs = [col(slab, k) for k in range(M.N_COLS)]
ins = np.asarray(prog.instrs, np.uint32).reshape(-1, 4)
stores = ins[(ins[:, 0] == ap.T_STORE) | (ins[:, 0] == ap.T_STORE_IF)]
n_loaded, n_stored = len(set(ins[ins[:, 0] == ap.LOAD][:, 2])), len(set(stores[:, 2]))
assert (n_loaded, n_stored) == (M.N_SEED, n_out)


def once(call):
    hip_chk(hip.hipEventRecord(ev0, stream))
    call()
    hip_chk(hip.hipEventRecord(ev1, stream))
    hip_chk(hip.hipEventSynchronize(ev1))
    t = C.c_float()
    hip_chk(hip.hipEventElapsedTime(C.byref(t), ev0, ev1))
    return t.value


def summary(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3)}


def variant(flag):
    def run():
        be.set_option("trace.vec4", flag)
        be.trace_program(prog, ptrs, log)
    return run


# the produced columns as a host would send them: the checked prefix repeated (the upload's cost does not depend on the values)
derived_u8 = [np.resize(np.asarray(w[:CHECKED], np.uint8), n) for w in want[M.N_SEED:]]
d8 = be.columns(n_out, log)
a8, k8 = nz._narrow_columns(derived_u8)
t8 = (C.c_void_p * len(a8))(*[col(d8, k) for k in range(len(a8))])
candidates = {
    "fill_one_row_per_lane": variant(0),
    "fill_four_positions_per_lane": variant(1),
    "nx_copy_of_the_stored_words": lambda: be._chk(be.L.nx_copy(be.ctx, dst.ptr, C.c_void_p(col(slab, M.N_SEED)), C.c_size_t(n_stored * n))),
    "narrow_upload_of_the_produced_columns_u8": lambda: be._chk(be.L.nx_upload_columns_narrow(be.ctx, *nz._host_columns(a8, k8), len(a8), log, t8, 0)),
}
out = {"tool": "rv32m_bench", "log_size": log, "rounds": rounds, "seed_columns": n_loaded, "produced_columns": n_stored, "instructions": int(len(ins)),
       "stored_words": n_stored * n}
with step("compile + check", 400):
    for name in ("fill_one_row_per_lane", "fill_four_positions_per_lane"):
        be._chk(be.L.nx_memset_zero(be.ctx, C.c_void_p(col(slab, M.N_SEED)), C.c_size_t(n_out * n)))
        candidates[name]()
        got = nz.DeviceColumns.view(be, col(slab, M.N_SEED), n_out, log).to_cpu()
        out[name] = {"equals_model_on_first_rows": bool(all(np.array_equal(g[:CHECKED], np.asarray(w[:CHECKED], np.uint32)) for g, w in zip(got, want[M.N_SEED:])))}
        del got
with step("timing", 400):
    ms = {name: [] for name in candidates}
    for r in range(rounds + 1):
        for name, call in candidates.items():
            t = once(call)
            if r:
                ms[name].append(t)
be.set_option("trace.vec4", 1)
for name in candidates:
    out.setdefault(name, {}).update(summary(ms[name]))
default = "fill_four_positions_per_lane"                       # what a context runs unless "trace.vec4" is cleared
out["four_over_one"] = round(out[default]["median_ms"] / out["fill_one_row_per_lane"]["median_ms"], 3)
for name in ("fill_one_row_per_lane", default):
    out[name]["over_nx_copy"] = round(out[name]["median_ms"] / out["nx_copy_of_the_stored_words"]["median_ms"], 3)
    out[name]["narrow_upload_over_it"] = round(out["narrow_upload_of_the_produced_columns_u8"]["median_ms"] / out[name]["median_ms"], 2)
out["narrow_upload_of_the_produced_columns_u8"]["host_bytes"] = n_stored * n
be.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "rv32m_bench.json"), "w") as f:
    f.write(line + "\n")
print(line)
