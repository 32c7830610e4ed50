"""nx_trace_program at the row-local chips' shape: at 2^22 rows a byte-limb add, a shift decomposition and a bitwise chip derive 29
output columns from 12 seed columns (two 4-byte operands, a shift amount, three opcode flags), next to the two yardsticks:
  nx_copy of the same number of column words — the streaming bound of this box for the bytes the kernel moves — and
  nx_upload_columns_narrow of the 29 derived columns as NX_COL_U8 — what a host that derives them itself pays to send them.
nx_trace_program is timed in both kernel shapes (context option "trace.vec4": one row per lane, four storage positions per lane).
Every figure is HIP-event time on the context's stream around the whole call, warmed, the candidates alternating round by round in one
process.
  timeout -k 10 600 python tools/trace_program_bench.py [log=22] [rounds=7]
Every step runs under a deadline of its own: a step that exceeds it ends the process (exit status 124) before anything else is
started on the GPU.  Writes profiles/trace_program_bench.json and prints the same line."""
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
import nexus_zkvm_amd.air_program as ap

log = int(sys.argv[1]) if len(sys.argv) > 1 else 22
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
n = 1 << log
B, Cc, SH, F_ADD, F_SLL, F_XOR, N_SEED = 0, 4, 8, 9, 10, 11, 12
VA, CARRY, S, H1, E, REM, QT, AND, OR, N_COLS = 12, 16, 18, 23, 24, 25, 29, 33, 37, 41


class step:
    """`with step(name, seconds):` — the deadline of one step."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def expired():
            sys.stderr.write(f"trace_program_bench: step '{self.name}' exceeded {self.seconds} s\n")
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


def chips():
    """AddChip (byte limbs, carries at the 16-bit boundaries), SllChip (shift bits, Helper1, Exp1_3, remainder and quotient limbs) and a
    bitwise chip (AND / OR helpers, XOR result); the three share ValueA, each on the rows of its own flag."""
    pb = ap.ProgramBuilder()
    col = lambda k: pb.next_trace_mask(k)[0]
    b, c, sh = [col(B + k) for k in range(4)], [col(Cc + k) for k in range(4)], col(SH)
    f_add, f_sll, f_xor = col(F_ADD), col(F_SLL), col(F_XOR)
    lo = b[0] + c[0] + (b[1] + c[1]) * 256
    carry0 = pb.shr(lo, 16)
    hi = b[2] + c[2] + (b[3] + c[3]) * 256 + carry0
    pb.store(CARRY, carry0)
    pb.store(CARRY + 1, pb.shr(hi, 16))
    for k, v in enumerate((pb.band(lo, 255), pb.band(pb.shr(lo, 8), 255), pb.band(hi, 255), pb.band(pb.shr(hi, 8), 255))):
        pb.store_if(f_add, VA + k, v)
    for k in range(5):
        pb.store(S + k, pb.band(pb.shr(sh, k), 1))
    pb.store(H1, pb.shl(1, pb.band(sh, 3)))
    e = pb.shl(1, pb.band(sh, 7))
    pb.store(E, e)
    rem, qt = [pb.band(b[k] * e, 255) for k in range(4)], [pb.shr(b[k] * e, 8) for k in range(4)]
    for k in range(4):
        pb.store(REM + k, rem[k])
        pb.store(QT + k, qt[k])
        pb.store_if(f_sll, VA + k, rem[k] + qt[k - 1] if k else rem[k])
    for k in range(4):
        pb.store(AND + k, pb.band(b[k], c[k]))
        pb.store(OR + k, pb.bor(b[k], c[k]))
        pb.store_if(f_xor, VA + k, pb.bxor(b[k], c[k]))
    return pb.build_trace_program()


def expected(seed):
    """the 29 derived columns by numpy, row by row (the program is row-local: any row order)"""
    t = [np.asarray(s, np.uint32) for s in seed] + [None] * (N_COLS - N_SEED)
    b, c, sh = t[B:B + 4], t[Cc:Cc + 4], t[SH]
    lo = b[0] + c[0] + 256 * (b[1] + c[1])
    hi = b[2] + c[2] + 256 * (b[3] + c[3]) + (lo >> 16)
    add = [lo & 255, (lo >> 8) & 255, hi & 255, (hi >> 8) & 255]
    t[CARRY], t[CARRY + 1] = lo >> 16, hi >> 16
    for k in range(5):
        t[S + k] = (sh >> k) & 1
    t[H1], t[E] = np.uint32(1) << (sh & 3), np.uint32(1) << (sh & 7)
    for k in range(4):
        t[REM + k], t[QT + k] = (b[k] * t[E]) & 255, (b[k] * t[E]) >> 8
        t[AND + k], t[OR + k] = b[k] & c[k], b[k] | c[k]
    for k in range(4):
        sll = t[REM + k] + (t[QT + k - 1] if k else 0)
        t[VA + k] = np.where(t[F_ADD] == 1, add[k], np.where(t[F_SLL] == 1, sll, b[k] ^ c[k]))
    return [np.asarray(x, np.uint32) for x in t[N_SEED:]]


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
    slab, dst = be.columns(N_COLS, log), be.columns(N_COLS, log)
col = lambda d, k: d.ptr.value + k * (4 << log)

with step("seeds", 120):
    rng = np.random.default_rng(22)
    owner = rng.integers(0, 3, n)
    seed = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(8)] + [rng.integers(0, 32, n, dtype=np.uint8)] + [(owner == k).astype(np.uint8) for k in range(3)]
    arrs, kinds = nz._narrow_columns(seed)
    table = (C.c_void_p * N_SEED)(*[col(slab, k) for k in range(N_SEED)])
    be._chk(be.L.nx_upload_columns_narrow(be.ctx, *nz._host_columns(arrs, kinds), N_SEED, log, table, 0))
    want = expected(seed)
    derived_u8 = [w.astype(np.uint8) for w in want]
    assert all(np.array_equal(w, d) for w, d in zip(want, derived_u8))      # every derived column is a byte column

prog = chips()
ptrs = [col(slab, k) for k in range(N_COLS)]
ins = np.asarray(prog.instrs, np.uint32).reshape(-1, 4)
stores = ins[(ins[:, 0] == ap.T_STORE) | (ins[:, 0] == ap.T_STORE_IF)]
n_loaded, n_stored = len(set(ins[ins[:, 0] == ap.LOAD][:, 2])), len(set(stores[:, 2]))
assert (n_loaded, n_stored) == (N_SEED, N_COLS - N_SEED)
moved_cols = n_loaded + n_stored                       # column words the kernel must move: every seed read once, every output written once
copy_words = moved_cols * n // 2                       # nx_copy reads and writes each word: the same number of column words in all


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


d8 = be.columns(N_COLS - N_SEED, log)
a8, k8 = nz._narrow_columns(derived_u8)
t8 = (C.c_void_p * len(a8))(*[col(d8, k) for k in range(len(a8))])
candidates = {
    "one_row_per_lane": variant(0),
    "four_positions_per_lane": variant(1),
    "nx_copy_same_column_words": lambda: be._chk(be.L.nx_copy(be.ctx, dst.ptr, slab.ptr, C.c_size_t(copy_words))),
    "narrow_upload_of_the_derived_columns_u8": lambda: be._chk(be.L.nx_upload_columns_narrow(be.ctx, *nz._host_columns(a8, k8), len(a8), log, t8, 0)),
}
out = {"tool": "trace_program_bench", "log_size": log, "rounds": rounds, "seed_columns": n_loaded, "derived_columns": n_stored, "instructions": int(len(ins)),
       "bytes_moved": 4 * moved_cols * n}
with step("compile + check", 300):
    for name in ("one_row_per_lane", "four_positions_per_lane"):
        be._chk(be.L.nx_memset_zero(be.ctx, C.c_void_p(col(slab, N_SEED)), C.c_size_t((N_COLS - N_SEED) * n)))
        candidates[name]()
        got = nz.DeviceColumns.view(be, col(slab, N_SEED), N_COLS - N_SEED, log).to_cpu()
        out[name] = {"equals_numpy": bool(all(np.array_equal(g, w) for g, w in zip(got, want)))}
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
for name in ("one_row_per_lane", "four_positions_per_lane", "nx_copy_same_column_words"):
    out[name]["GBs_moved"] = round(out["bytes_moved"] / out[name]["median_ms"] / 1e6, 1)
out["narrow_upload_of_the_derived_columns_u8"]["host_bytes"] = n_stored * n
best = min(("one_row_per_lane", "four_positions_per_lane"), key=lambda k: out[k]["median_ms"])
out["faster_variant"] = best
out["four_over_one"] = round(out["four_positions_per_lane"]["median_ms"] / out["one_row_per_lane"]["median_ms"], 3)
out["trace_program_over_copy"] = round(out[best]["median_ms"] / out["nx_copy_same_column_words"]["median_ms"], 3)
out["narrow_upload_over_trace_program"] = round(out["narrow_upload_of_the_derived_columns_u8"]["median_ms"] / out[best]["median_ms"], 1)
be.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "trace_program_bench.json"), "w") as f:
    f.write(line + "\n")
print(line)
