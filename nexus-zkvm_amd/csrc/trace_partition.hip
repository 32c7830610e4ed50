// The step table of an execution split into per-opcode component traces on the device.
//
// Every execution component of the reference's v2 prover takes the steps of its own opcode only (ExecutionComponent::iter_program_steps,
// prover2/machine/src/components/execution/common/mod.rs:31-39): row i of the component is the i-th such step, the trace is padded to a
// power of two with IsLocalPad = 1 (execution/add/mod.rs:157-183); the Cpu component takes every step (components/cpu/trace.rs:36-59).
// That is a stable multi-way partition of the steps followed by a gather into bit-reversed circle-domain order:
//   order      ONE counting pass of count_pass.cuh over the class column (histogram, scan, stable placement) with the policy TpOrder:
//              the digit is the class, n_classes histogram rows, order[class_start[c] + rank] = step.  A step of class NX_PART_NONE is no
//              element; a class word that is neither that nor below n_classes is no element either and leaves its step in a 32-bit minimum.
//   fill       one work-item per storage position of one destination: it derives its natural row r once, reads the row's step from the
//              order (class_start + r; the row itself for NX_PART_ALL), loads every source word the destination uses ONCE and cuts all
//              limbs of that word from the register.  The destination's descriptor, its limb specs and its column pointers are
//              wave-uniform: they are read through the constant address space (written before the launch, never by it), so they are
//              scalar loads and every column leaves as a single-word store at the lane's byte offset from an SGPR base.
// Blocks communicate at kernel boundaries only: nothing waits on another block.  Every sum is an integer sum, every word is the same on
// every run.
#include "internal.h"
#include <algorithm>
#include <string.h>
#include <string>

namespace nx {

#include "trace_rows.h"
#include "count_pass.cuh"

constexpr u32 TP_THREADS = CP_THREADS;
constexpr u32 TP_MAX_CLASSES = NX_PART_MAX_CLASSES, TP_MAX_STEPS = 1u << 30;
constexpr size_t TP_MAX_TABLE_BYTES = (size_t)1 << 20;       // descriptors of one fill launch (a call with more is cut between destinations)

struct TpCtl { u32 first_bad, total, pad[2]; u32 start[TP_MAX_CLASSES]; };
struct TpDest { u32 start, count, log_size, all, n_groups, group_at, col_at, pad; u32* is_pad; u32* step; };
struct TpGroup { u32 src, n_limbs, limb_at, pad; };          // limb_at: first limb of the group among the destination's (col_at + limb_at)
struct TpLimb { u32 shift, mask; };

#ifndef NX_TP_HOST_SHIM
// Uniform data of a launch, read through the constant address space: a scalar load.
#define TP_CONSTANT __attribute__((address_space(4)))
template <class T> __device__ __forceinline__ T tp_uniform(const T* p) { return *(TP_CONSTANT const T*)p; }
// word at (uniform base) + a 32-bit byte offset, and the store of one: `global_load_dword v, v_off, s[base]` / `global_store_dword v_off, v, s[base]`
__device__ __forceinline__ u32 tp_load(const u32* base, u32 byte_off) { return *(NX_GLOBAL_AS const u32*)((NX_GLOBAL_AS const char*)base + byte_off); }
__device__ __forceinline__ void tp_store(u32* base, u32 byte_off, u32 w) { *(NX_GLOBAL_AS u32*)((NX_GLOBAL_AS char*)base + byte_off) = w; }
// The offset as a value the CURRENT basic block defines: across a loop that is not unrolled its zero extension is hoisted, the offset
// arrives as a 64-bit pair and every store pays a 64-bit add (KrDevStore::here).  Emits nothing.
__device__ __forceinline__ u32 tp_here(u32 off) { asm volatile("" : "+v"(off)); return off; }
#endif

// the order as a counting pass: step j is an element if its class word is below n_classes; the histogram walk reports a word outside the
// classes that is not NX_PART_NONE, the placement stores the step index
struct TpOrder {
    const u32* cls; u32 n_classes; u32* first_bad; u32* order;
    typedef u32 Item;
    __device__ __forceinline__ bool class_of(u32 j, u32 n_steps, u32* c, bool report) const {
        *c = 0;
        if (j >= n_steps) return false;
        const u32 w = gld(cls + j);
        if (w < n_classes) { *c = w; return true; }
        if (report && w != NX_PART_NONE) atomicMin(first_bad, j);
        return false;
    }
    __device__ __forceinline__ bool digit(u32 j, u32 n_steps, u32* c) const { return class_of(j, n_steps, c, true); }
    __device__ __forceinline__ bool load(u32 j, u32 n_steps, Item* it, u32* c) const { *it = j; return class_of(j, n_steps, c, false); }
    __device__ __forceinline__ void store(u32 slot, const Item& it) const { gst(order + slot, it); }
};

// last index i < n with a[i] <= x (a ascending, a[0] <= x); a and x are uniform over the block
__device__ __forceinline__ u32 tp_find(const u32* a, u32 n, u32 x) {
    u32 lo = 0, hi = n;
    while (hi - lo > 1) { const u32 mid = (lo + hi) / 2; if (tp_uniform(a + mid) <= x) lo = mid; else hi = mid; }
    return lo;
}

// One block per tile of 256 storage positions of one destination; tile_start: first tile of every one.
__global__ __launch_bounds__(TP_THREADS) void tp_fill_kernel(const TpDest* __restrict__ dests, const u32* __restrict__ tile_start, u32 n_dests, const TpGroup* __restrict__ groups,
                                                             const TpLimb* __restrict__ limbs, u32* const* __restrict__ cols, const u32* const* __restrict__ srcs,
                                                             const u32* __restrict__ order) {
    const u32 d = tp_find(tile_start, n_dests, blockIdx.x);
    const TpDest* __restrict__ Dp = dests + d;       // read field by field: every one a scalar load
    TpDest D;
    D.start = tp_uniform(&Dp->start); D.count = tp_uniform(&Dp->count); D.log_size = tp_uniform(&Dp->log_size); D.all = tp_uniform(&Dp->all);
    D.n_groups = tp_uniform(&Dp->n_groups); D.group_at = tp_uniform(&Dp->group_at); D.col_at = tp_uniform(&Dp->col_at);
    D.is_pad = tp_uniform(&Dp->is_pad); D.step = tp_uniform(&Dp->step);
    const u32 idx = (blockIdx.x - tp_uniform(tile_start + d)) * TP_THREADS + threadIdx.x, n = 1u << D.log_size;
    if (idx >= n) return;
    // by storage position: the stores of a wave are 256 consecutive bytes of every column, the reads are gathered.  Walking by natural
    // row (r = idx, pos = pos_of_coset_row(r)) coalesces the reads and scatters the stores, and took 2.4x to 3.7x as long (DESIGN §6
    // item 71).
    const u32 pos = idx, r = coset_row_of_pos(pos, (int)D.log_size);
    const bool real = r < D.count;
    u32 step = 0;
    if (real) step = D.all ? r : gld(order + D.start + r);
    const u32 off = pos * 4;                        // < 2^32: log_size <= 30
    if (D.is_pad) tp_store(D.is_pad, off, real ? 0u : 1u);
    if (D.step) tp_store(D.step, off, step);
    for (u32 g = 0; g < D.n_groups; g++) {
        const TpGroup* __restrict__ Gp = groups + D.group_at + g;
        const u32 g_src = tp_uniform(&Gp->src), g_limbs = tp_uniform(&Gp->n_limbs), g_at = D.col_at + tp_uniform(&Gp->limb_at);
        u32 w = 0;
        if (real) w = tp_load(tp_uniform(srcs + g_src), tp_here(step * 4));  // step < 2^30
        for (u32 l = 0; l < g_limbs; l++) {
            const u32 at = g_at + l;
            const u32 v = (w >> tp_uniform(&limbs[at].shift)) & tp_uniform(&limbs[at].mask);
            tp_store(tp_uniform(cols + at), tp_here(off), v == P ? 0u : v);
        }
    }
}

}  // namespace nx

using namespace nx;

struct nx_partition {
    nx_ctx* ctx;
    const u32* d_class;
    u32 n_steps, n_classes;
    u32* d_order;                       // n_steps words from the context's allocator (NULL for an empty table)
    std::vector<u32> start;             // n_classes + 1 offsets into d_order; host memory
};

extern "C" {

uint32_t nx_trace_partition_log_size(uint64_t count, uint32_t min_log) {
    u32 log = 0;
    while (log < 63 && ((u64)1 << log) < count) log++;
    return std::max(log, min_log);
}

int nx_trace_partition_create(nx_ctx* ctx, const uint32_t* d_class, uint32_t n_steps, uint32_t n_classes, uint32_t* counts, nx_partition** out) {
    NX_GUARD(ctx);
    const std::string who = "nx_trace_partition_create";
    // every refusal is decided from host memory alone; the NULL context comes last so that each of them can be met without a device
    if (!out) return set_err(ctx, NX_ERR_ARG, who + ": NULL out");
    if (!counts) return set_err(ctx, NX_ERR_ARG, who + ": NULL counts");
    if (n_classes < 1 || n_classes > TP_MAX_CLASSES) return set_err(ctx, NX_ERR_ARG, who + ": n_classes of " + std::to_string(n_classes) + ", 1 to 256");
    if (n_steps > TP_MAX_STEPS) return set_err(ctx, NX_ERR_ARG, who + ": n_steps of " + std::to_string(n_steps) + ", at most 2^30");
    if (n_steps && !d_class) return set_err(ctx, NX_ERR_ARG, who + ": NULL d_class with n_steps of " + std::to_string(n_steps));
    if (!ctx) return set_err(ctx, NX_ERR_ARG, who + ": NULL context");
    *out = nullptr;

    std::unique_ptr<nx_partition> p(new nx_partition());
    p->ctx = ctx; p->d_class = d_class; p->n_steps = n_steps; p->n_classes = n_classes; p->d_order = nullptr;
    p->start.assign(n_classes + 1, 0);
    if (n_steps) {
        const CountPlan plan = count_plan(n_steps);
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t b_ctl = al(sizeof(TpCtl)), b_hist = al((size_t)n_classes * plan.blocks * 4);
        NX_TRY(dev_alloc(ctx, (size_t)n_steps * 4, (void**)&p->d_order));
        uint8_t* blob = nullptr;
        int rc = dev_alloc(ctx, b_ctl + b_hist, (void**)&blob);
        if (rc != NX_OK) { dev_free(ctx, p->d_order); return rc; }
        TpCtl* d_ctl = (TpCtl*)blob; u32* d_hist = (u32*)(blob + b_ctl); u32* d_order = p->d_order;
        TpCtl h_ctl; memset(&h_ctl, 0, sizeof h_ctl); h_ctl.first_bad = 0xFFFFFFFFu;
        rc = upload_async_staged(ctx, d_ctl, &h_ctl, sizeof h_ctl);
        hipError_t e = hipSuccess;
        if (rc == NX_OK) {
            const TpOrder order = {d_class, n_classes, &d_ctl->first_bad, d_order};
            e = count_pass(ctx, order, n_steps, plan, n_classes, d_hist, &d_ctl->total, d_ctl->start);
            if (e == hipSuccess) rc = copy_d2h_blocking(ctx, &h_ctl, d_ctl, sizeof h_ctl);
        }
        // The copy above blocks, so every launch has completed.  Where a launch failed the copy is skipped and earlier kernels may still
        // run: the blocks then go back to the context's cache, whose reuse is ordered on ctx->stream behind them.
        dev_free(ctx, blob);
        if (e != hipSuccess || rc != NX_OK) {
            dev_free(ctx, p->d_order);
            return e != hipSuccess ? hip_fail(ctx, e, who.c_str(), __FILE__, __LINE__) : rc;
        }
        if (h_ctl.first_bad != 0xFFFFFFFFu) {
            dev_free(ctx, p->d_order);
            *out = nullptr;
            u32 word = 0;
            NX_TRY(copy_d2h_blocking(ctx, &word, d_class + h_ctl.first_bad, 4));
            return set_err(ctx, NX_ERR_PROTOCOL, who + ": step " + std::to_string(h_ctl.first_bad) + ": class " + std::to_string(word) + ", " + std::to_string(n_classes) + " classes");
        }
        for (u32 c = 0; c < n_classes; c++) p->start[c] = h_ctl.start[c];
        p->start[n_classes] = h_ctl.total;
    }
    for (u32 c = 0; c < n_classes; c++) counts[c] = p->start[c + 1] - p->start[c];
    *out = p.release();
    return NX_OK;
}

void nx_trace_partition_destroy(nx_partition* part) {
    if (!part) return;
    NX_GUARD(part->ctx);
    if (part->d_order) dev_free(part->ctx, part->d_order);
    delete part;
}

int nx_trace_partition_fill(nx_ctx* ctx, const nx_partition* part, const uint32_t* const* d_src, uint32_t n_src, const nx_part_dest* dests, uint32_t n_dests) {
    NX_GUARD(ctx);
    const std::string who = "nx_trace_partition_fill";
    if (!part) return set_err(ctx, NX_ERR_ARG, who + ": NULL partition");
    if (!ctx || ctx != part->ctx) return set_err(ctx, NX_ERR_ARG, who + (ctx ? ": the partition belongs to another context" : ": NULL context"));
    if (n_dests && !dests) return set_err(ctx, NX_ERR_ARG, who + ": NULL dests");
    if (n_src && !d_src) return set_err(ctx, NX_ERR_ARG, who + ": NULL d_src");
    const u32 n_classes = part->n_classes, n_steps = part->n_steps;

    std::vector<TpDest> h_dest(n_dests);
    std::vector<u32> h_tile(n_dests + 1, 0);
    std::vector<TpGroup> h_group;
    std::vector<TpLimb> h_limb;
    std::vector<u32*> h_col;
    std::vector<std::pair<const void*, std::string>> outs;
    std::vector<const void*> ins;
    if (part->d_class) ins.push_back(part->d_class);
    for (u32 s = 0; s < n_src; s++) if (d_src[s]) ins.push_back(d_src[s]);
    u64 tiles = 0;
    for (u32 i = 0; i < n_dests; i++) {
        const nx_part_dest& s = dests[i];
        const std::string at = who + ": destination " + std::to_string(i);
        const bool all = s.cls == NX_PART_ALL;
        if (!all && s.cls >= n_classes) return set_err(ctx, NX_ERR_ARG, at + ": class " + std::to_string(s.cls) + ", " + std::to_string(n_classes) + " classes");
        if (s.log_size < 1 || s.log_size > 30) return set_err(ctx, NX_ERR_ARG, at + ": log_size of " + std::to_string(s.log_size) + ", 1 to 30");
        const u32 count = all ? n_steps : part->start[s.cls + 1] - part->start[s.cls];
        if (((u64)1 << s.log_size) < count)
            return set_err(ctx, NX_ERR_ARG, at + ": log_size of " + std::to_string(s.log_size) + ", its " + std::to_string(count) + " steps do not fit 2^" + std::to_string(s.log_size));
        if (s.n_cols && !s.d_cols) return set_err(ctx, NX_ERR_ARG, at + ": NULL d_cols");
        if (s.n_cols && !s.limbs) return set_err(ctx, NX_ERR_ARG, at + ": NULL limbs");
        TpDest& D = h_dest[i]; memset(&D, 0, sizeof D);
        D.start = all ? 0 : part->start[s.cls]; D.count = count; D.log_size = s.log_size; D.all = all;
        D.group_at = (u32)h_group.size(); D.col_at = (u32)h_col.size(); D.is_pad = s.d_is_pad; D.step = s.d_step;
        // the specs grouped by source (a stable sort: columns of one source keep the caller's order)
        std::vector<u32> by_src(s.n_cols);
        for (u32 c = 0; c < s.n_cols; c++) {
            const nx_part_limb& l = s.limbs[c];
            const std::string col = at + " column " + std::to_string(c);
            if (l.src >= n_src) return set_err(ctx, NX_ERR_ARG, col + ": src of " + std::to_string(l.src) + ", " + std::to_string(n_src) + " source columns");
            if (l.bits < 1 || l.bits > 31 || l.shift > 31 || l.shift + l.bits > 32)
                return set_err(ctx, NX_ERR_ARG, col + ": shift " + std::to_string(l.shift) + " bits " + std::to_string(l.bits) + ", 1 <= bits <= 31 and shift + bits <= 32");
            if (n_steps && !d_src[l.src]) return set_err(ctx, NX_ERR_ARG, col + ": d_src[" + std::to_string(l.src) + "] is NULL");
            if (!s.d_cols[c]) return set_err(ctx, NX_ERR_ARG, col + ": NULL output column");
            outs.push_back({s.d_cols[c], col});
            by_src[c] = c;
        }
        if (s.d_is_pad) outs.push_back({s.d_is_pad, at + " d_is_pad"});
        if (s.d_step) outs.push_back({s.d_step, at + " d_step"});
        std::stable_sort(by_src.begin(), by_src.end(), [&](u32 a, u32 b) { return s.limbs[a].src < s.limbs[b].src; });
        for (u32 k = 0; k < s.n_cols; k++) {
            const nx_part_limb& l = s.limbs[by_src[k]];
            if (!k || l.src != s.limbs[by_src[k - 1]].src) { TpGroup G; G.src = l.src; G.n_limbs = 0; G.limb_at = k; G.pad = 0; h_group.push_back(G); D.n_groups++; }
            h_group.back().n_limbs++;
            TpLimb L; L.shift = l.shift; L.mask = (u32)(((u64)1 << l.bits) - 1);
            h_limb.push_back(L); h_col.push_back(s.d_cols[by_src[k]]);
        }
        tiles += (((u64)1 << s.log_size) + TP_THREADS - 1) / TP_THREADS;
        if (tiles >= ((u64)1 << 31)) return set_err(ctx, NX_ERR_ARG, who + ": 2^39 rows or more in all (destination " + std::to_string(i) + ")");
    }
    {
        std::sort(ins.begin(), ins.end());
        std::sort(outs.begin(), outs.end());
        for (size_t i = 0; i < outs.size(); i++) {
            if (i && outs[i].first == outs[i - 1].first) return set_err(ctx, NX_ERR_ARG, outs[i].second + " has the pointer of" + outs[i - 1].second.substr(who.size() + 1));
            if (std::binary_search(ins.begin(), ins.end(), outs[i].first)) return set_err(ctx, NX_ERR_ARG, outs[i].second + " has the pointer of a source or class column");
        }
    }
    if (!n_dests) return NX_OK;

    // the source pointers once, then the destinations in launches of at most TP_MAX_TABLE_BYTES of descriptors
    std::vector<const u32*> h_src(std::max<u32>(1, n_src), nullptr);
    for (u32 s = 0; s < n_src; s++) h_src[s] = d_src[s];
    for (u32 i0 = 0; i0 < n_dests;) {
        u32 i1 = i0;
        size_t bytes = 0;
        while (i1 < n_dests) {
            const u32 g1 = i1 + 1 < n_dests ? h_dest[i1 + 1].group_at : (u32)h_group.size(), c1 = i1 + 1 < n_dests ? h_dest[i1 + 1].col_at : (u32)h_col.size();
            const size_t add = sizeof(TpDest) + 4 + (g1 - h_dest[i1].group_at) * sizeof(TpGroup) + (c1 - h_dest[i1].col_at) * (sizeof(TpLimb) + sizeof(u32*));
            if (i1 > i0 && bytes + add > TP_MAX_TABLE_BYTES) break;
            bytes += add; i1++;
        }
        const u32 nd = i1 - i0, g0 = h_dest[i0].group_at, c0 = h_dest[i0].col_at;
        const u32 ng = (i1 < n_dests ? h_dest[i1].group_at : (u32)h_group.size()) - g0, nc = (i1 < n_dests ? h_dest[i1].col_at : (u32)h_col.size()) - c0;
        // one staged block: pointers first (8-byte aligned), then the words
        auto al8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
        const size_t o_src = 0, o_col = o_src + h_src.size() * sizeof(u32*), o_dest = o_col + (size_t)nc * sizeof(u32*), o_group = o_dest + (size_t)nd * sizeof(TpDest),
                     o_limb = o_group + (size_t)ng * sizeof(TpGroup), o_tile = o_limb + (size_t)nc * sizeof(TpLimb), total = al8(o_tile + (size_t)(nd + 1) * 4);
        std::vector<uint8_t> blob(total, 0);
        memcpy(blob.data() + o_src, h_src.data(), h_src.size() * sizeof(u32*));
        if (nc) memcpy(blob.data() + o_col, h_col.data() + c0, (size_t)nc * sizeof(u32*));
        std::vector<u32> tile(nd + 1, 0);
        for (u32 k = 0; k < nd; k++) {
            TpDest D = h_dest[i0 + k]; D.group_at -= g0; D.col_at -= c0;
            memcpy(blob.data() + o_dest + (size_t)k * sizeof(TpDest), &D, sizeof D);
            tile[k + 1] = tile[k] + (u32)((((u64)1 << D.log_size) + TP_THREADS - 1) / TP_THREADS);
        }
        if (ng) memcpy(blob.data() + o_group, h_group.data() + g0, (size_t)ng * sizeof(TpGroup));
        if (nc) memcpy(blob.data() + o_limb, h_limb.data() + c0, (size_t)nc * sizeof(TpLimb));
        memcpy(blob.data() + o_tile, tile.data(), (size_t)(nd + 1) * 4);
        uint8_t* staged = nullptr;
        NX_TRY(stage(ctx, blob.data(), total, (void**)&staged));
        hipLaunchKernelGGL(tp_fill_kernel, dim3(tile[nd]), dim3(TP_THREADS), 0, ctx->stream, (const TpDest*)(staged + o_dest), (const u32*)(staged + o_tile), nd,
                           (const TpGroup*)(staged + o_group), (const TpLimb*)(staged + o_limb), (u32* const*)(staged + o_col), (const u32* const*)(staged + o_src),
                           (const u32*)part->d_order);
        NX_LAUNCH_CHECK(ctx);
        i0 = i1;
    }
    return NX_OK;
}

}  // extern "C"
