// The main and preprocessed trace of the reference's PermutationMemoryCheck component, filled on the device from what an instance
// consists of: its 200-byte input state, one address and 200 timestamps (prover/src/extensions/keccak/memory_check/trace.rs:32-123,
// which runs a full keccakf per row on the CPU).  out_state is keccak-f[1600] of the row's input, which no row program computes; here a
// work-item owns one storage position, loads its instance's 25 lanes, and runs the 24 rounds of keccak_round.h untraced in 64-bit
// registers.  Every column leaves as single-word stores at the lane's byte offset: consecutive lanes of a wave store consecutive words
// of one column, the column pointer is wave-uniform (a scalar load from the table through the constant address space: the table is
// written before the launch and never by it).  The timestamps of a row arrive as 16-byte loads.  The column emitter is
// keccak_memcheck.h.
#include "internal.h"
#include <algorithm>
#include <string>

namespace nx {

#include "trace_rows.h"
#include "keccak_round.h"
#include "keccak_memcheck.h"
#include "keccak_store.h"

static_assert(KM_MAIN_COLS == NX_KECCAK_MEMCHECK_MAIN_COLS && KM_PRE_COLS == NX_KECCAK_MEMCHECK_PRE_COLS, "keccak_memcheck.h and nexus_hip.h disagree");

// one wave per block: a trace of 2^14 rows is 256 waves, which 256-thread blocks would put on 64 of the 256 CUs
constexpr u32 KM_THREADS = 64;
// quads: the row's 200 timestamps as 50 16-byte words (d_timestamps is 16-byte aligned and a row is 800 bytes); NULL on a padding row
typedef u32 KmQuad __attribute__((ext_vector_type(4)));
struct KmDevTimestamps {
    const KmQuad* quads;
    __device__ __forceinline__ void ts4(u32 j, u32 (&w)[4]) const {
        KmQuad v = {0, 0, 0, 0};
        if (quads) v = *(NX_GLOBAL_AS const KmQuad*)(quads + j);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
};

// table: KM_MAIN_COLS main column pointers, then (has_pre) KM_PRE_COLS preprocessed ones
__global__ __launch_bounds__(KM_THREADS) void keccak_memcheck_kernel(const u64* __restrict__ states, const u32* __restrict__ addresses, const u32* __restrict__ timestamps,
                                                                     u32 n_instances, int log_size, u32* const* __restrict__ table, u32 has_pre, u64* __restrict__ states_out) {
    const u32 pos = blockIdx.x * KM_THREADS + threadIdx.x, n = 1u << log_size;
    if (pos >= n) return;
    const u32 r = coset_row_of_pos(pos, log_size);      // natural row r is instance r
    const bool real = r < n_instances;
    u64 a[KR_LANES];
#pragma unroll
    for (u32 l = 0; l < KR_LANES; l++) a[l] = real ? kr_gld64(states + (size_t)r * KR_LANES + l) : 0;
    const u32 addr = real ? *(NX_GLOBAL_AS const u32*)(addresses + r) : 0;
    const KmDevTimestamps ts{real ? (const KmQuad*)(timestamps + (size_t)r * KM_STATE) : nullptr};
    const KrDevStore main{(NX_KR_CONSTANT const KrColumn*)table, pos * 4}, pre{(NX_KR_CONSTANT const KrColumn*)(table + KM_MAIN_COLS), pos * 4};
    km_fill_row(main, pre, has_pre != 0, a, addr, ts, !real, r == n - 1);
    if (states_out && real) {
#pragma unroll
        for (u32 l = 0; l < KR_LANES; l++) kr_gst64(states_out + (size_t)r * KR_LANES + l, a[l]);
    }
}

}  // namespace nx

using namespace nx;

extern "C" int nx_trace_keccak_memory_check(nx_ctx* ctx, const uint64_t* d_states, const uint32_t* d_addresses, const uint32_t* d_timestamps, uint32_t n_instances,
                                            uint32_t log_size, uint32_t* const* d_main, uint32_t* const* d_pre, uint64_t* d_states_out) {
    NX_GUARD(ctx);
    const std::string who = "nx_trace_keccak_memory_check";
    // every refusal is decided from host memory alone; the NULL context comes last so that each of them can be met without a device
    if (log_size < 1 || log_size > 30) return set_err(ctx, NX_ERR_ARG, who + ": log_size of " + std::to_string(log_size) + ", 1 to 30");
    if ((u64)n_instances > ((u64)1 << log_size))
        return set_err(ctx, NX_ERR_ARG, who + ": n_instances of " + std::to_string(n_instances) + ": one row each, they do not fit 2^" + std::to_string(log_size));
    if (!d_main) return set_err(ctx, NX_ERR_ARG, who + ": NULL d_main");
    std::vector<std::pair<const void*, u32>> ptrs;      // (pointer, index; d_pre's behind d_main's)
    const u32 n_cols = KM_MAIN_COLS + (d_pre ? KM_PRE_COLS : 0);
    auto name = [](u32 k) { return k < KM_MAIN_COLS ? "d_main[" + std::to_string(k) + "]" : "d_pre[" + std::to_string(k - KM_MAIN_COLS) + "]"; };
    for (u32 k = 0; k < n_cols; k++) {
        const void* p = k < KM_MAIN_COLS ? d_main[k] : d_pre[k - KM_MAIN_COLS];
        if (!p) return set_err(ctx, NX_ERR_ARG, who + ": " + name(k) + " is NULL");
        ptrs.push_back({p, k});
    }
    std::sort(ptrs.begin(), ptrs.end());
    for (size_t k = 1; k < ptrs.size(); k++)
        if (ptrs[k].first == ptrs[k - 1].first)
            return set_err(ctx, NX_ERR_ARG, who + ": " + name(ptrs[k].second) + " has the pointer of " + name(ptrs[k - 1].second));
    if (n_instances && !d_states) return set_err(ctx, NX_ERR_ARG, who + ": NULL d_states with n_instances of " + std::to_string(n_instances));
    if (n_instances && !d_addresses) return set_err(ctx, NX_ERR_ARG, who + ": NULL d_addresses with n_instances of " + std::to_string(n_instances));
    if (n_instances && !d_timestamps) return set_err(ctx, NX_ERR_ARG, who + ": NULL d_timestamps with n_instances of " + std::to_string(n_instances));
    if ((uintptr_t)d_states & 7) return set_err(ctx, NX_ERR_ARG, who + ": d_states is not 8-byte aligned");
    if ((uintptr_t)d_states_out & 7) return set_err(ctx, NX_ERR_ARG, who + ": d_states_out is not 8-byte aligned");
    if ((uintptr_t)d_timestamps & 15) return set_err(ctx, NX_ERR_ARG, who + ": d_timestamps is not 16-byte aligned");
    const uintptr_t state_bytes = (uintptr_t)n_instances * KR_LANES * sizeof(u64);
    if (d_states && d_states_out && (uintptr_t)d_states_out < (uintptr_t)d_states + state_bytes && (uintptr_t)d_states < (uintptr_t)d_states_out + state_bytes)
        return set_err(ctx, NX_ERR_ARG, who + ": d_states_out overlaps d_states");
    if (!ctx) return set_err(ctx, NX_ERR_ARG, who + ": NULL context");

    // the pointer table travels through the context's staging ring, as nx_trace_keccak_round's does: no device allocation
    std::vector<u32*> h_table(KM_MAIN_COLS + KM_PRE_COLS, nullptr);
    std::copy(d_main, d_main + KM_MAIN_COLS, h_table.begin());
    if (d_pre) std::copy(d_pre, d_pre + KM_PRE_COLS, h_table.begin() + KM_MAIN_COLS);
    void* staged = nullptr;
    NX_TRY(stage(ctx, h_table.data(), h_table.size() * sizeof(u32*), &staged));
    const u32 n = 1u << log_size;
    hipLaunchKernelGGL(keccak_memcheck_kernel, dim3((n + KM_THREADS - 1) / KM_THREADS), dim3(KM_THREADS), 0, ctx->stream, (const u64*)d_states, (const u32*)d_addresses,
                       (const u32*)d_timestamps, n_instances, (int)log_size, (u32* const*)staged, d_pre ? 1u : 0u, (u64*)d_states_out);
    NX_LAUNCH_CHECK(ctx);
    return NX_OK;
}
