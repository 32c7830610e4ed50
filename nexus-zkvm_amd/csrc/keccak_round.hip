// The main and preprocessed trace of the reference's KeccakRound component, filled on the device from the instances' input states
// (prover/src/extensions/keccak/round/trace.rs:240-366: convert_input_to_simd, generate_round_component_trace).  Row i of an instance
// holds the state after i rounds, so the 200 seed columns are not row-local and nx_trace_program cannot fill them; here a work-item
// owns one storage position, loads its instance's 25 lanes, runs i untraced rounds in 64-bit registers and then the traced one, whose
// every intermediate lane leaves as 8 single-word stores: consecutive lanes of a wave store consecutive words of one column, the column
// pointer is wave-uniform (a scalar load from the table through the constant address space: the table is written before the launch and
// never by it).  The work-items of an instance's last row write d_states_out: no second pass, no scratch buffer.  The round and the
// column emitter are keccak_round.h.
#include "internal.h"
#include <algorithm>
#include <string>

namespace nx {

#include "trace_rows.h"
#include "keccak_round.h"
#include "keccak_store.h"

static_assert(KR_MAIN_COLS == NX_KECCAK_ROUND_MAIN_COLS && KR_PRE_COLS == NX_KECCAK_ROUND_PRE_COLS, "keccak_round.h and nexus_hip.h disagree");

constexpr u32 KR_THREADS = 256;
// table: KR_MAIN_COLS main column pointers, then (has_pre) KR_PRE_COLS preprocessed ones
__global__ __launch_bounds__(KR_THREADS) void keccak_round_kernel(const u64* __restrict__ states, u32 n_instances, u32 first_round, u32 log_rounds, int log_size,
                                                                  u32* const* __restrict__ table, u32 has_pre, u64* __restrict__ states_out) {
    const u32 pos = blockIdx.x * KR_THREADS + threadIdx.x, n = 1u << log_size;
    if (pos >= n) return;
    const u32 r = coset_row_of_pos(pos, log_size), rounds = 1u << log_rounds, i = r & (rounds - 1), inst = r >> log_rounds;
    const bool real = inst < n_instances;
    u64 a[KR_LANES];
#pragma unroll
    for (u32 l = 0; l < KR_LANES; l++) a[l] = real ? kr_gld64(states + (size_t)inst * KR_LANES + l) : 0;
    const KrDevStore main{(NX_KR_CONSTANT const KrColumn*)table, pos * 4}, pre{(NX_KR_CONSTANT const KrColumn*)(table + KR_MAIN_COLS), pos * 4};
    kr_fill_row(main, pre, has_pre != 0, a, i, first_round, rounds, !real, r == n - 1);
    if (states_out && real && i == rounds - 1) {
#pragma unroll
        for (u32 l = 0; l < KR_LANES; l++) kr_gst64(states_out + (size_t)inst * KR_LANES + l, a[l]);
    }
}

}  // namespace nx

using namespace nx;

extern "C" int nx_trace_keccak_round(nx_ctx* ctx, const uint64_t* d_states, uint32_t n_instances, uint32_t first_round, uint32_t log_rounds, uint32_t log_size,
                                     uint32_t* const* d_main, uint32_t* const* d_pre, uint64_t* d_states_out) {
    NX_GUARD(ctx);
    const std::string who = "nx_trace_keccak_round";
    // every refusal is decided from host memory alone; the NULL context comes last so that each of them can be met without a device
    if (log_rounds > 4 || first_round > KR_MAX_ROUNDS || first_round + (1u << log_rounds) > KR_MAX_ROUNDS)
        return set_err(ctx, NX_ERR_ARG, who + ": first_round of " + std::to_string(first_round) + " and log_rounds of " + std::to_string(log_rounds) + ": first_round + 2^log_rounds is above 24");
    if (log_size < 1 || log_size > 30) return set_err(ctx, NX_ERR_ARG, who + ": log_size of " + std::to_string(log_size) + ", 1 to 30");
    if (((u64)n_instances << log_rounds) > ((u64)1 << log_size))
        return set_err(ctx, NX_ERR_ARG, who + ": n_instances of " + std::to_string(n_instances) + ": " + std::to_string((u64)n_instances << log_rounds) + " rows do not fit 2^" + std::to_string(log_size));
    if (!d_main) return set_err(ctx, NX_ERR_ARG, who + ": NULL d_main");
    std::vector<std::pair<const void*, u32>> ptrs;      // (pointer, index; d_pre's behind d_main's)
    const u32 n_cols = KR_MAIN_COLS + (d_pre ? KR_PRE_COLS : 0);
    auto name = [](u32 k) { return k < KR_MAIN_COLS ? "d_main[" + std::to_string(k) + "]" : "d_pre[" + std::to_string(k - KR_MAIN_COLS) + "]"; };
    for (u32 k = 0; k < n_cols; k++) {
        const void* p = k < KR_MAIN_COLS ? d_main[k] : d_pre[k - KR_MAIN_COLS];
        if (!p) return set_err(ctx, NX_ERR_ARG, who + ": " + name(k) + " is NULL");
        ptrs.push_back({p, k});
    }
    std::sort(ptrs.begin(), ptrs.end());
    for (size_t k = 1; k < ptrs.size(); k++)
        if (ptrs[k].first == ptrs[k - 1].first)
            return set_err(ctx, NX_ERR_ARG, who + ": " + name(ptrs[k].second) + " has the pointer of " + name(ptrs[k - 1].second));
    if (n_instances && !d_states) return set_err(ctx, NX_ERR_ARG, who + ": NULL d_states with n_instances of " + std::to_string(n_instances));
    if ((uintptr_t)d_states & 7) return set_err(ctx, NX_ERR_ARG, who + ": d_states is not 8-byte aligned");
    if ((uintptr_t)d_states_out & 7) return set_err(ctx, NX_ERR_ARG, who + ": d_states_out is not 8-byte aligned");
    const uintptr_t state_bytes = (uintptr_t)n_instances * KR_LANES * sizeof(u64);
    if (d_states && d_states_out && (uintptr_t)d_states_out < (uintptr_t)d_states + state_bytes && (uintptr_t)d_states < (uintptr_t)d_states_out + state_bytes)
        return set_err(ctx, NX_ERR_ARG, who + ": d_states_out overlaps d_states");
    if (!ctx) return set_err(ctx, NX_ERR_ARG, who + ": NULL context");

    // the pointer table travels through the context's staging ring, as nx_trace_program's does: no device allocation
    std::vector<u32*> h_table(KR_MAIN_COLS + KR_PRE_COLS, nullptr);
    std::copy(d_main, d_main + KR_MAIN_COLS, h_table.begin());
    if (d_pre) std::copy(d_pre, d_pre + KR_PRE_COLS, h_table.begin() + KR_MAIN_COLS);
    void* staged = nullptr;
    NX_TRY(stage(ctx, h_table.data(), h_table.size() * sizeof(u32*), &staged));
    const u32 n = 1u << log_size;
    hipLaunchKernelGGL(keccak_round_kernel, dim3((n + KR_THREADS - 1) / KR_THREADS), dim3(KR_THREADS), 0, ctx->stream, (const u64*)d_states, n_instances, first_round, log_rounds,
                       (int)log_size, (u32* const*)staged, d_pre ? 1u : 0u, (u64*)d_states_out);
    NX_LAUNCH_CHECK(ctx);
    return NX_OK;
}
