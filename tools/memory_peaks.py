"""The peak of the context's block allocator (nx_ctx_memory with reset_peak) for the statements the benchmarks run, into
profiles/memory_peaks.json (one JSON document, also printed):
  * the benchmark statements at bench.py's sizes: the headline machine (2^22 rows x 27 + 347 + 64 columns), the v1 shape (the same
    trace with 250 logup columns = 1000 interaction columns, bound 2, plus 8 small components) and the keccak shape
    (tools/keccak_shaped.py);
  * nx_prover_check on a committed session statement;
  * the trace entries at the sizes of their tools/*_bench.py, on zero-filled (or counting) inputs: their temporaries follow the shapes,
    not the values;
  * the v1 shape at every doubling of the row count, and from the last doubling's slope a MODEL of the largest v1-shaped log_n_rows
    whose peak stays under the card's 288 GB.  It is an extrapolation: nothing is run at a size that was not run before.
Every figure is live bytes of BLOCKS: the context's fixed buffers (16 MiB staging ring, pinned host rings) are not blocks.  "peak" is the
high-water mark during the call, "inputs" what the caller held when it began, "temporaries" their difference.
usage: memory_peaks.py [--shift S] [--skip-doublings] [--out FILE]     --shift: every log size reduced by S bits (a quick look)"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
CARD_BYTES = 288 * 10**9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shift", type=int, default=0)
    ap.add_argument("--skip-doublings", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memory_peaks.json"))
    a = ap.parse_args()
    import numpy as np
    import nexus_zkvm_amd as nz
    from keccak_shaped import keccak_shaped_components
    S = a.shift
    be = nz.HipBackend(0)
    out = {"tool": "memory_peaks", "shift": S, "unit": "bytes of live allocator blocks", "statements": {}, "entries": {}}

    def measured(fn):
        """{"inputs", "peak", "temporaries"} around fn() — after one warm call, from an empty cache"""
        be.sync(); be.trim()
        live0, _ = be.memory(reset_peak=True)
        try:
            fn()
            be.sync()
        except nz.NexusHipError as e:
            if "HIP error" in str(e):
                raise
            return {"error": str(e)}
        _, peak = be.memory()
        return {"inputs": live0, "peak": peak, "temporaries": peak - live0}

    def peak_request(fn, peak):
        """which request takes the live count to its peak: the call again under a budget one rounding unit below the peak, which refuses
        exactly that request on the host (nothing more is asked of the driver than in the run before) -> its size and its position"""
        if not peak:
            return None
        c0 = be.get_option("debug.alloc_count")
        be.set_option("mem.limit_bytes", peak - 256)
        try:
            fn()
            text = None
        except nz.NexusHipError as e:
            text = str(e)
        finally:
            be.set_option("mem.limit_bytes", 0)
        if not text or "(mem.limit_bytes)" not in text:
            return {"error": text}
        pos = be.get_option("debug.alloc_count") - c0
        c0 = be.get_option("debug.alloc_count")
        fn()
        return {"bytes": int(text.split("dev_alloc: ")[1].split(" bytes refused")[0]), "live_before_it": int(text.split("refused: ")[1].split(" live of")[0]),
                "position": pos, "requests_of_the_call": be.get_option("debug.alloc_count") - c0}

    def zeros(n_cols, log):
        d = be.columns(n_cols, log)
        be._chk(be.L.nx_memset_zero(be.ctx, d.ptr, C.c_size_t(n_cols << log)))
        return d

    def ptrs(d, first=0, n=None):
        n = d.n_cols - first if n is None else n
        return [d.ptr.value + (first + i) * (4 << d.log_size) for i in range(n)]

    # ---- the benchmark statements
    L = 22 - S
    v1 = lambda log: [(log, 27, 347, 1000, 2)] + [(max(2, 8 + k - S), 2, 6 + k, 4, 1) for k in range(8)]      # noqa: E731
    statements = {
        "headline (2^%d rows x 438 columns, bound 1)" % L: ([(L, 27, 347, 64)], nz.default_config(pow_bits=10)),
        "v1 shape (2^%d rows x 1374 columns, bound 2, 8 small components)" % L: (v1(L), nz.default_config(pow_bits=10, log_constraint_degree=2)),
        "keccak shape (round components of 2^%d and 2^%d rows)" % (18 - S, 17 - S): (keccak_shaped_components(S), nz.default_config(pow_bits=10)),
    }
    for name, (comps, cfg) in statements.items():
        be.prove_machine(comps, cfg, seed=5)                     # kernels compiled
        r = measured(lambda: be.prove_machine(comps, cfg, seed=5))
        r["request_that_reaches_the_peak"] = peak_request(lambda: be.prove_machine(comps, cfg, seed=5), r.get("peak"))
        r["trace_cells"] = sum((c[1] + c[2] + c[3]) << c[0] for c in comps)
        r["bytes_per_trace_cell"] = round(r["peak"] / r["trace_cells"], 2) if "peak" in r else None
        out["statements"][name] = r
        print(name, r, flush=True)

    # ---- the v1 shape at every doubling, and the model
    if not a.skip_doublings:
        cfg = nz.default_config(pow_bits=10, log_constraint_degree=2)
        series = {}
        for log in range(max(10, 16 - S), L + 1):
            be.prove_machine(v1(log), cfg, seed=5)
            series[log] = measured(lambda: be.prove_machine(v1(log), cfg, seed=5)).get("peak")
        logs = sorted(series)
        out["v1_shape_peak_by_log_n_rows"] = {str(k): series[k] for k in logs}
        out["v1_shape_peak_ratio_per_doubling"] = {str(k): round(series[k] / series[k - 1], 3) for k in logs[1:] if series[k] and series[k - 1]}
        if len(logs) >= 2 and series[logs[-1]] and series[logs[-2]]:
            slope = (series[logs[-1]] - series[logs[-2]]) / float((1 << logs[-1]) - (1 << logs[-2]))        # bytes per row, from the last doubling
            fixed = series[logs[-1]] - slope * (1 << logs[-1])
            fit = logs[-1]
            while fixed + slope * (1 << (fit + 1)) < CARD_BYTES:
                fit += 1
            out["model"] = {"label": "MODEL, not a measurement: peak(log) = fixed + bytes_per_row * 2^log from the last two measured doublings", "bytes_per_row": round(slope, 1),
                            "fixed_bytes": round(fixed), "card_bytes": CARD_BYTES, "largest_v1_shaped_log_n_rows_under_the_card": fit,
                            "modelled_peak_there": round(fixed + slope * (1 << fit)), "modelled_peak_one_doubling_further": round(fixed + slope * (1 << (fit + 1)))}
        print(out.get("model"), flush=True)

    # ---- nx_prover_check on a committed session statement (the synthetic AIR, one component)
    import nexus_zkvm_amd.air_program as airp
    import air_examples as AE
    import oracle_lib as O
    O.build_oracle()
    log, n_pre, n_main, n_inter = max(6, 16 - S), 4, 24, 8
    comps1 = [(log, n_pre, n_main, n_inter)]
    ss = be.prover_session(nz.default_config(pow_bits=10), log)
    ss.mix_u64(log)
    ss.commit(O.synth_tree_columns(comps1, 0, 1)); ss.commit(O.synth_tree_columns(comps1, 1, 1))
    ss.mix_felts(np.zeros(4, np.uint32))
    ss.commit(O.synth_tree_columns(comps1, 2, 1, inter_seed=5))
    comp = AE.synthetic_component(airp, log, n_pre, n_main, n_inter)
    assert ss.check([comp]).ok
    out["entries"]["nx_prover_check (2^%d rows x %d columns; inputs: the committed session)" % (log, n_pre + n_main + n_inter)] = measured(lambda: ss.check([comp]))
    ss.close()

    # ---- the trace entries at the sizes of their bench tools
    T = 22 - S
    n = 1 << T

    def entry(name, fn, before=None):
        try:
            fn()                                  # warm
        except nz.NexusHipError as e:
            if "HIP error" in str(e):
                raise
        if before:
            before()
        out["entries"][name] = measured(fn)
        print(name, out["entries"][name], flush=True)

    # nx_logup_multiplicities: 340 byte-limb columns against a 256-row range table
    uses_d = zeros(340, T)
    table = be.columns_from_host(np.arange(256, dtype=np.uint32)[None, :])
    mult = zeros(1, 8)
    entry("nx_logup_multiplicities (340 columns of 2^%d rows, 256-row table)" % T,
          lambda: be.logup_multiplicities([([p], None, T) for p in ptrs(uses_d)], ptrs(table), 8, [8], mult.ptr.value, want_rc=True))
    uses_d = None
    # nx_logup_multiplicities_sparse: uses of 2^T rows keyed by two 16-bit limbs against 2^(T-2) table rows
    LT = max(2, T - 2)
    keys = np.arange(1 << LT, dtype=np.uint64) * 4093          # distinct 32-bit addresses, spread over the key space
    tcols = be.columns_from_host(np.stack([(keys & 0xFFFF).astype(np.uint32), (keys >> 16).astype(np.uint32)]))
    use2, mult2 = zeros(2, T), zeros(1, LT)
    entry("nx_logup_multiplicities_sparse (one use of 2^%d rows, 2^%d table rows, keys [16, 16])" % (T, LT),
          lambda: be.logup_multiplicities_sparse([(ptrs(use2), None, T)], ptrs(tcols), None, LT, [16, 16], mult2.ptr.value, want_rc=True))
    tcols = use2 = mult2 = None
    # nx_trace_prev_access / nx_trace_access_chain: 4 byte streams of 2^T rows, 32-bit address as 4 byte limbs, 2 payload columns
    ins, outs = [zeros(7, T) for _ in range(4)], [zeros(3, T) for _ in range(4)]
    streams = [{"key": ptrs(i, 0, 4), "flag": None, "payload": ptrs(i, 5, 2), "prev": ptrs(o, 0, 2), "ordinal": ptrs(o, 2, 1)[0], "log_size": T, "epoch": 0, "linear": False} for i, o in zip(ins, outs)]
    entry("nx_trace_prev_access (4 streams of 2^%d rows, keys [8, 8, 8, 8], 2 payload columns)" % T, lambda: be.trace_prev_access(streams, [8, 8, 8, 8], 2, init=[0, 0], want_rc=True))
    entry("nx_trace_access_chain (the same 4 column streams)", lambda: be.trace_access_chain(streams, [8, 8, 8, 8], 2, init=[0, 0], want_rc=True))
    ins = outs = streams = None
    # nx_trace_partition_create / _fill: 2^T steps, 8 source columns, 40 classes (every step in class 0: one destination of 2^T rows)
    cls, src = zeros(1, T), zeros(8, T)
    limbs = [(s, sh, 8) for s in range(8) for sh in (0, 8, 16, 24)]
    dst = zeros(len(limbs) + 1, T)
    held = {}

    def create():
        held["counts"], held["part"] = be.trace_partition(cls.ptr.value, n, 40)
    entry("nx_trace_partition_create (2^%d steps, 40 classes; the peak includes the handle's order column)" % T, create, before=lambda: held.pop("part").destroy())
    entry("nx_trace_partition_fill (8 source columns into %d limb columns of class 0)" % len(limbs),
          lambda: held["part"].fill(ptrs(src), [{"cls": 0, "log_size": T, "cols": ptrs(dst, 0, len(limbs)), "limbs": limbs, "is_pad": ptrs(dst, len(limbs), 1)[0], "step": None}]))
    held.pop("part").destroy()
    cls = src = dst = None
    # nx_trace_keccak_round / nx_trace_keccak_memory_check: 2^14 instances
    import keccak_memcheck_model as KMM
    import keccak_round_model as KRM
    li = max(2, 14 - S)
    ni = 1 << li
    states = zeros(1, max(1, int(50 * ni - 1).bit_length()))
    sout = zeros(1, states.log_size)
    main = zeros(KRM.MAIN_COLS, li + 4)
    entry("nx_trace_keccak_round (2^%d instances x 16 rounds, 2^%d rows x %d columns)" % (li, li + 4, KRM.MAIN_COLS),
          lambda: be.trace_keccak_round(states.ptr.value, ni, 0, 4, li + 4, ptrs(main), None, sout.ptr.value))
    main = zeros(KMM.MAIN_COLS, li)
    addr, ts = zeros(1, li), zeros(1, max(1, int(200 * ni - 1).bit_length()))
    entry("nx_trace_keccak_memory_check (2^%d instances, %d columns)" % (li, KMM.MAIN_COLS),
          lambda: be.trace_keccak_memory_check(states.ptr.value, addr.ptr.value, ts.ptr.value, ni, li, ptrs(main), None, sout.ptr.value))
    main = states = sout = addr = ts = None

    be.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
