"""The narrow host-trace upload against the u32 one: one session tree of 347 columns at 2^22 rows — 340 byte limbs and
7 full-field columns, config #2's byte-limb width — committed from host memory in both host orders through
  u32          commit_host with uint32 arrays (every byte crosses PCIe as four),
  u8           commit_host_narrow with uint8 arrays for the limbs (sent as they are, widened on the device),
  packed_tN    commit_host_narrow with the uint32 arrays and as_kind=uint8 (packed on N host threads: host.pack_threads = 1 / 4 / 8 / 16),
and nx_upload_columns_narrow's rate for the same columns.  Every variant is warmed up, then the variants alternate for `rounds` rounds;
the line reports min / median / max commit times, the roots of all variants per order and whether they are equal.
  python tools/narrow_upload_bench.py [log_size=22] [rounds=3]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import nexus_zkvm_amd as nz  # noqa: E402

log = int(sys.argv[1]) if len(sys.argv) > 1 else 22
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N_LIMB, N_FULL = 340, 7
n = 1 << log
rng = np.random.default_rng(66)
limb8 = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(N_LIMB)]
full = [rng.integers(0, nz.P, n, dtype=np.uint32) for _ in range(N_FULL)]
limb32 = [c.astype(np.uint32) for c in limb8]
cols32 = limb32 + full                 # the reference's layout: every column uint32
cols8 = limb8 + full
as_kind = [np.uint8] * N_LIMB + [None] * N_FULL
be = nz.HipBackend(0)
cfg = nz.default_config(pow_bits=4)
THREADS = (1, 4, 8, 16)


def commit(variant, coset_order):
    s = be.prover_session(cfg, log)
    try:
        be.sync()
        if variant.startswith("packed_t"):
            be.set_option("host.pack_threads", int(variant[len("packed_t"):]))
        t0 = time.perf_counter()
        if variant == "u32":
            root, _ = s.commit_host(cols32, coset_order=coset_order)
        elif variant == "u8":
            root, _ = s.commit_host_narrow(cols8, coset_order=coset_order)
        else:
            root, _ = s.commit_host_narrow(cols32, coset_order=coset_order, as_kind=as_kind)
        ms = (time.perf_counter() - t0) * 1e3
    finally:
        s.close()
    return ms, "".join("%08x" % w for w in root)


variants = ["u32", "u8"] + ["packed_t%d" % t for t in THREADS]
out = {"tool": "narrow_upload_bench", "log_size": log, "columns": N_LIMB + N_FULL, "byte_limb_columns": N_LIMB, "rounds": rounds,
       "host_bytes_u32": (N_LIMB + N_FULL) * 4 * n, "host_bytes_narrow": (N_LIMB + 4 * N_FULL) * n}
for coset_order in (False, True):
    order = "coset_order" if coset_order else "circle_order"
    roots, times = {}, {v: [] for v in variants}
    for v in variants:                                   # warm-up: code objects, the staging ring, the context's block cache
        _, roots[v] = commit(v, coset_order)
    for r in range(rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            ms, root = commit(v, coset_order)
            times[v].append(ms)
            assert root == roots[v], (order, v)
    res = {}
    for v in variants:
        t = sorted(times[v])
        res[v] = {"min_ms": round(t[0], 2), "median_ms": round(t[len(t) // 2], 2), "max_ms": round(t[-1], 2)}
        res[v]["vs_u32"] = round(t[len(t) // 2] / sorted(times["u32"])[len(t) // 2], 3)
    out[order] = {"commit": res, "roots": roots, "roots_equal": len(set(roots.values())) == 1}
be.set_option("host.pack_threads", 16)
# nx_upload_columns_narrow alone: the same columns into device columns (no transforms)
for name, cols, kind in (("upload_u32", cols32, None), ("upload_u8", cols8, None), ("upload_packed_t16", cols32, as_kind)):
    best = 1e9
    for _ in range(rounds + 1):
        be.sync()
        t0 = time.perf_counter()
        d = be.upload_columns_narrow(cols, coset_order=False, as_kind=kind)
        best = min(best, time.perf_counter() - t0)
        d.free()
    sent = out["host_bytes_u32"] if name == "upload_u32" else out["host_bytes_narrow"]
    out[name] = {"best_ms": round(best * 1e3, 2), "GBs_sent": round(sent / best / 1e9, 2), "GBs_u32_equivalent": round(out["host_bytes_u32"] / best / 1e9, 2)}
out["roots_equal"] = out["circle_order"]["roots_equal"] and out["coset_order"]["roots_equal"]
be.close()
print(json.dumps(out))
