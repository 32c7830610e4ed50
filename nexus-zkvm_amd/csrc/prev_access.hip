// Memory-checking columns on the device: for every access, what the previous access to the same address left behind.
//
// The reference walks the accesses in time order over a map (RegisterMemCheckSideNote::access, prover/src/trace/regs.rs:29-37;
// ReadWriteMemCheckSideNote::last_access, prover/src/trace/sidenote/mod.rs:25-47; program_mem_check.rs:49-96) and reads the final
// state tables off the map at the end.  Ordered by (key, time) it is one data-parallel problem:
//   enumerate  one element per (row, stream), written at its TIME INDEX (epoch, natural row, stream): the packed key and a 32-bit
//              handle (first element of the stream + storage position); a row that does not access, or holds an entry outside its
//              key_bits (recorded: min (stream << 32 | position)), gets the handle PA_NONE, which the last sort pass puts behind
//              every key.  The zeros of the rows that do not access are written here.
//   sort       stable LSD radix sort of the (key, handle) pairs, 8-bit digits: every pass is the counting pass of count_pass.cuh
//              (histogram, scan, stable placement) with the policy PaSort, which takes the digit from the key and moves the pair.
//   resolve    in sorted order element j continues the run of j - 1 or heads a new one: heads are counted and the last head is
//              found per block, both scanned over the blocks (one block), then every element gathers the payload of j - 1 (or
//              init), writes it with its ordinal j - head to its own storage position; heads and tails write the summary entry of
//              their run (index = heads before it; the keys are already ascending).
// Blocks communicate at kernel boundaries only: nothing waits on another block.  Atomics carry integers (LDS histogram adds, one
// 64-bit minimum for a bad row).
#include "internal.h"
#include <algorithm>
#include <string.h>
#include <string>

namespace nx {

#include "trace_rows.h"
#include "count_pass.cuh"

constexpr u32 PA_THREADS = CP_THREADS, PA_ENUM_TILE = PA_THREADS * 4, PA_RES_TILE = PA_THREADS * 4;
constexpr u32 PA_NONE = 0xFFFFFFFFu;                             // handle of an element that is no access (handles are < 2^31)
constexpr u32 PA_MAX_STREAMS = 1u << 16, PA_MAX_PAYLOAD = 16;

struct PaStream {
    const u32* key[4]; const u32* flag; u32* ord;
    u32 log_size, linear, vec, epoch_slot;
    uint16_t before_ge[32];     // earlier streams of the same epoch with log_size >= L (at most 65535)
};
// streams of one epoch: ge[b] of them have >= 2^b rows, the others have small[b] rows together; base: first time index of the epoch
struct PaEpoch { u32 base, ge[32], small[32]; };
struct PaPass { u32 shift, last, sentinel; };                    // digit = (key >> shift) & 255; in the last pass PA_NONE -> sentinel
struct PaInit { u32 w[PA_MAX_PAYLOAD]; };
struct PaSum { u32 cap; u32* key; u32* count; u32* last[PA_MAX_PAYLOAD]; };
struct PaCtl { u64 first_bad; u32 n_keys; u32 pad[13]; };       // one 64-byte block of device memory

__device__ __forceinline__ u32 pa_bitlen(u32 x) { return x ? 32u - (u32)__builtin_clz(x) : 0u; }

// One block per tile of 1024 storage positions of one stream (tile_start: first tile of every stream), four consecutive positions
// per lane.
__global__ __launch_bounds__(PA_THREADS) void pa_enumerate_kernel(const PaStream* __restrict__ streams, const PaEpoch* __restrict__ epochs, const u32* __restrict__ tile_start,
                                                                  const u32* __restrict__ sbase, u32 n_streams, PackedKey K, u32 n_payload, u32* const* __restrict__ prv,
                                                                  u32* __restrict__ keys, u32* __restrict__ vals, PaCtl* __restrict__ ctl) {
    const u32 s = find_le(tile_start, n_streams, blockIdx.x);
    const PaStream& S = streams[s];                 // read where it is: a per-lane copy would put before_ge, indexed at run time, into scratch
    const PaEpoch* __restrict__ E = epochs + S.epoch_slot;
    const u32 n = 1u << S.log_size;
    const u32 row0 = (blockIdx.x - tile_start[s]) * PA_ENUM_TILE + threadIdx.x * 4;
    if (row0 >= n) return;
    const bool vec = S.vec != 0;
    u32 k[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
#pragma unroll
    for (u32 c = 0; c < 4; c++)
        if (c < K.n_cols) {
            const uint4 v = gld4_guarded(S.key[c], row0, n, vec);
            const u32 x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (u32 e = 0; e < 4; e++) { k[e] |= x[e] << K.shift[c]; o[e] |= K.bits[c] < 32 ? x[e] >> K.bits[c] : 0u; }
        }
    uint4 fv = make_uint4(1, 1, 1, 1);
    if (S.flag) fv = gld4_guarded(S.flag, row0, n, vec);
    const u32 f[4] = {fv.x, fv.y, fv.z, fv.w};
    const u32 base = gld(sbase + s), ebase = E->base;
#pragma unroll
    for (u32 e = 0; e < 4; e++) {
        const u32 pos = row0 + e;
        if (pos >= n) break;
        const u32 r = S.linear ? pos : coset_row_of_pos(pos, (int)S.log_size);
        const u32 b = r ? pa_bitlen(r - 1) : 0;
        // elements of the epoch before natural row r: sum over its streams of min(r, rows); then the earlier streams that have row r
        const u32 idx = ebase + r * E->ge[b] + E->small[b] + S.before_ge[pa_bitlen(r)];
        const bool access = f[e] != 0, bad = access && o[e] != 0, ok = access && !bad;
        if (bad) atomicMin((unsigned long long*)&ctl->first_bad, ((unsigned long long)s << 32) | pos);
        gst(keys + idx, ok ? k[e] : 0u);
        gst(vals + idx, ok ? base + pos : PA_NONE);
    }
    if (!S.flag) return;
    // rows that do not access: zeros in every output of the stream
    if (vec && !(f[0] | f[1] | f[2] | f[3])) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        if (S.ord) gst4(S.ord + row0, z);
        for (u32 c = 0; c < n_payload; c++) { u32* p = prv[(size_t)s * n_payload + c]; if (p) gst4(p + row0, z); }
        return;
    }
    for (u32 e = 0; e < 4; e++) {
        const u32 pos = row0 + e;
        if (pos >= n || f[e]) continue;
        if (S.ord) gst(S.ord + pos, 0u);
        for (u32 c = 0; c < n_payload; c++) { u32* p = prv[(size_t)s * n_payload + c]; if (p) gst(p + pos, 0u); }
    }
}

__device__ __forceinline__ u32 pa_digit(u32 key, u32 val, PaPass ps) {
    const u32 d = ps.shift < 32 ? (key >> ps.shift) & 255u : 0u;
    return (ps.last && val == PA_NONE) ? ps.sentinel : d;
}

// one pass of the sort as a counting pass: the histogram needs the handle in the last pass only, the placement moves the pair
struct PaSort {
    const u32* kin; const u32* vin; u32* kout; u32* vout; PaPass ps;
    struct Item { u32 key, val; };
    __device__ __forceinline__ bool digit(u32 j, u32 total, u32* d) const {
        const bool have = j < total;
        const u32 key = have ? gld(kin + j) : 0u, val = (have && ps.last) ? gld(vin + j) : 0u;
        *d = have ? pa_digit(key, val, ps) : 0u;
        return have;
    }
    __device__ __forceinline__ bool load(u32 j, u32 total, Item* it, u32* d) const {
        const bool have = j < total;
        it->key = have ? gld(kin + j) : 0u; it->val = have ? gld(vin + j) : 0u;
        *d = have ? pa_digit(it->key, it->val, ps) : 0u;
        return have;
    }
    __device__ __forceinline__ void store(u32 slot, const Item& it) const { gst(kout + slot, it.key); gst(vout + slot, it.val); }
};

// the four sorted elements j0 .. j0 + 3 of a lane with their neighbours: is[e] heads a run, tail[e] ends one
struct PaQuad { u32 key[4], val[4], prev_val; bool head[4], tail[4]; };
__device__ __forceinline__ void pa_load_quad(const u32* __restrict__ keys, const u32* __restrict__ vals, u32 total, u32 j0, bool want_tail, PaQuad* q) {
    const bool full = j0 + 3 < total;
    const uint4 kv = gld4_guarded(keys, j0, total, full), vv = gld4_guarded(vals, j0, total, full);
    q->key[0] = kv.x; q->key[1] = kv.y; q->key[2] = kv.z; q->key[3] = kv.w;
    q->val[0] = vv.x; q->val[1] = vv.y; q->val[2] = vv.z; q->val[3] = vv.w;
    u32 pk = 0, pv = PA_NONE;                                 // the element before: a PA_NONE neighbour never continues a run
    if (j0 > 0 && j0 < total) { pk = gld(keys + j0 - 1); pv = gld(vals + j0 - 1); }
    q->prev_val = pv;
    u32 nk = 0, nv = PA_NONE;
    if (want_tail && j0 + 4 < total) { nk = gld(keys + j0 + 4); nv = gld(vals + j0 + 4); }
#pragma unroll
    for (u32 e = 0; e < 4; e++) {
        const bool ok = j0 + e < total && q->val[e] != PA_NONE;
        const u32 bk = e ? q->key[e - 1] : pk, bv = e ? q->val[e - 1] : pv;
        const u32 ak = e < 3 ? q->key[e + 1] : nk, av = (e < 3 ? (j0 + e + 1 < total ? q->val[e + 1] : PA_NONE) : nv);
        q->head[e] = ok && (bv == PA_NONE || bk != q->key[e]);
        q->tail[e] = ok && (av == PA_NONE || ak != q->key[e]);
    }
}

// per block of 1024 sorted elements: the heads in it and (index + 1) of its last head, 0 = none
__global__ __launch_bounds__(PA_THREADS) void pa_heads_kernel(const u32* __restrict__ keys, const u32* __restrict__ vals, u32 total, u32* __restrict__ blk_cnt, u32* __restrict__ blk_last) {
    __shared__ u32 lds[4];
    const u32 j0 = blockIdx.x * PA_RES_TILE + threadIdx.x * 4;
    PaQuad q; pa_load_quad(keys, vals, total, j0, false, &q);
    u32 cnt = 0, last = 0;
#pragma unroll
    for (u32 e = 0; e < 4; e++) if (q.head[e]) { cnt++; last = j0 + e + 1; }
    u32 tc, tl;
    (void)block_scan<0>(cnt, lds, &tc);
    (void)block_scan<1>(last, lds, &tl);
    if (threadIdx.x == 0) { blk_cnt[blockIdx.x] = tc; blk_last[blockIdx.x] = tl; }
}

// blk_cnt / blk_last: scanned over the blocks (heads before the block; last head before the block).  sbase: first handle of every
// stream; pay / prv: [stream][payload column] pointer tables.
__global__ __launch_bounds__(PA_THREADS) void pa_resolve_kernel(const u32* __restrict__ keys, const u32* __restrict__ vals, u32 total, const u32* __restrict__ blk_cnt,
                                                                const u32* __restrict__ blk_last, const PaStream* __restrict__ streams, const u32* __restrict__ sbase, u32 n_streams,
                                                                u32 n_payload, const u32* const* __restrict__ pay, u32* const* __restrict__ prv, PaInit init, PaSum sum) {
    __shared__ u32 lds[4];
    const u32 j0 = blockIdx.x * PA_RES_TILE + threadIdx.x * 4;
    PaQuad q; pa_load_quad(keys, vals, total, j0, true, &q);
    u32 cnt = 0, last = 0;
#pragma unroll
    for (u32 e = 0; e < 4; e++) if (q.head[e]) { cnt++; last = j0 + e + 1; }
    u32 unused;
    u32 seg = blk_cnt[blockIdx.x] + block_scan<0>(cnt, lds, &unused);              // heads before this lane's elements
    u32 start = scan_op<1>(blk_last[blockIdx.x], block_scan<1>(last, lds, &unused)); // (index + 1) of the last head before them
    for (u32 e = 0; e < 4; e++) {
        const u32 j = j0 + e;
        // The rows that do not access are sorted last, so nothing follows the first PA_NONE.  One exception: a call without any d_flag
        // and with whole-byte keys has PA_NONE only on REFUSED rows, which share digit 255 with real keys; the call then returns
        // NX_ERR_PROTOCOL and its outputs are unspecified, and skipping the rest of the quad stays in bounds (find_le never sees PA_NONE).
        if (j >= total || q.val[e] == PA_NONE) break;
        if (q.head[e]) { seg++; start = j + 1; }
        const u32 run = seg - 1, ordinal = j + 1 - start;
        const u32 s = find_le(sbase, n_streams, q.val[e]), pos = q.val[e] - sbase[s];
        const u32 pval = e ? q.val[e - 1] : q.prev_val;
        u32 ps = 0, ppos = 0;
        if (!q.head[e]) { ps = find_le(sbase, n_streams, pval); ppos = pval - sbase[ps]; }
        u32* ord = streams[s].ord;
        if (ord) gst(ord + pos, ordinal);
        const bool to_sum = q.tail[e] && run < sum.cap;
        if (q.head[e] && run < sum.cap && sum.key) gst(sum.key + run, q.key[e]);
        if (to_sum && sum.count) gst(sum.count + run, ordinal + 1);
        for (u32 c = 0; c < n_payload; c++) {
            u32* dst = prv[(size_t)s * n_payload + c];
            if (dst) {
                u32 x = init.w[c];
                if (!q.head[e]) { const u32* src = pay[(size_t)ps * n_payload + c]; x = src ? gld(src + ppos) : 0u; }
                gst(dst + pos, x);
            }
            if (to_sum && sum.last[c]) { const u32* src = pay[(size_t)s * n_payload + c]; gst(sum.last[c] + run, src ? gld(src + pos) : 0u); }
        }
    }
}

}  // namespace nx

using namespace nx;

extern "C" {

int nx_trace_prev_access(nx_ctx* ctx, const nx_access_stream* streams, uint32_t n_streams, uint32_t n_key_cols, const uint32_t* key_bits,
                         uint32_t n_payload, const uint32_t* init, const nx_access_summary* summary, uint64_t* n_keys) {
    NX_GUARD(ctx);
    const std::string who = "nx_trace_prev_access";
    // every refusal is decided from host memory alone; the NULL context comes last so that each of them can be met without a device
    if (!streams) return set_err(ctx, NX_ERR_ARG, who + ": NULL streams");
    if (!key_bits) return set_err(ctx, NX_ERR_ARG, who + ": NULL key_bits");
    if (n_streams < 1 || n_streams > PA_MAX_STREAMS) return set_err(ctx, NX_ERR_ARG, who + ": n_streams of " + std::to_string(n_streams) + ", 1 to 65536");
    if (n_key_cols < 1 || n_key_cols > 4) return set_err(ctx, NX_ERR_ARG, who + ": n_key_cols of " + std::to_string(n_key_cols) + ", 1 to 4");
    if (n_payload < 1 || n_payload > PA_MAX_PAYLOAD) return set_err(ctx, NX_ERR_ARG, who + ": n_payload of " + std::to_string(n_payload) + ", 1 to 16");
    PackedKey K; memset(&K, 0, sizeof K);
    K.n_cols = n_key_cols;
    for (u32 c = 0; c < n_key_cols; c++) {
        if (key_bits[c] < 1 || key_bits[c] > 32) return set_err(ctx, NX_ERR_ARG, who + ": key_bits[" + std::to_string(c) + "] of " + std::to_string(key_bits[c]) + ", 1 to 32");
        K.bits[c] = key_bits[c]; K.shift[c] = K.total_bits; K.total_bits += key_bits[c];
        if (K.total_bits > 32) return set_err(ctx, NX_ERR_ARG, who + ": the key_bits add up to more than 32");
    }
    PaInit h_init; memset(&h_init, 0, sizeof h_init);
    for (u32 c = 0; init && c < n_payload; c++) {
        if (init[c] >= P) return set_err(ctx, NX_ERR_ARG, who + ": init[" + std::to_string(c) + "] is not below p");
        h_init.w[c] = init[c];
    }
    // streams: sizes, pointers, aliasing
    std::vector<const void*> ins, outs;
    u64 rows = 0;
    bool any_flag = false;
    for (u32 i = 0; i < n_streams; i++) {
        const nx_access_stream& s = streams[i];
        const std::string at = who + ": stream " + std::to_string(i);
        if (s.log_size > 30 || (!s.linear && s.log_size < 1))
            return set_err(ctx, NX_ERR_ARG, at + ": log_size of " + std::to_string(s.log_size) + (s.linear ? ", 0 to 30 for a linear stream" : ", 1 to 30"));
        rows += (u64)1 << s.log_size;
        if (rows >= ((u64)1 << 31)) return set_err(ctx, NX_ERR_ARG, who + ": 2^31 rows or more in all (log_size of stream " + std::to_string(i) + ")");
        if (!s.d_key) return set_err(ctx, NX_ERR_ARG, at + ": NULL d_key");
        for (u32 c = 0; c < n_key_cols; c++) {
            if (!s.d_key[c]) return set_err(ctx, NX_ERR_ARG, at + ": NULL d_key[" + std::to_string(c) + "]");
            ins.push_back(s.d_key[c]);
        }
        if (s.d_flag) { ins.push_back(s.d_flag); any_flag = true; }
        for (u32 c = 0; c < n_payload; c++) {
            if (s.d_payload && s.d_payload[c]) ins.push_back(s.d_payload[c]);
            if (s.d_prev && s.d_prev[c]) outs.push_back(s.d_prev[c]);
        }
        if (s.d_ordinal) outs.push_back(s.d_ordinal);
    }
    PaSum h_sum; memset(&h_sum, 0, sizeof h_sum);
    if (summary) {
        h_sum.cap = summary->cap; h_sum.key = summary->d_key; h_sum.count = summary->d_count;
        if (h_sum.key) outs.push_back(h_sum.key);
        if (h_sum.count) outs.push_back(h_sum.count);
        for (u32 c = 0; summary->d_last && c < n_payload; c++) { h_sum.last[c] = summary->d_last[c]; if (h_sum.last[c]) outs.push_back(h_sum.last[c]); }
    }
    {
        std::sort(ins.begin(), ins.end()); std::sort(outs.begin(), outs.end());
        for (size_t i = 0; i < outs.size(); i++)
            if ((i && outs[i] == outs[i - 1]) || std::binary_search(ins.begin(), ins.end(), outs[i]))
                return set_err(ctx, NX_ERR_ARG, who + ": an output column (d_prev, d_ordinal or summary) has the pointer of another column of the call");
    }
    if (!ctx) return set_err(ctx, NX_ERR_ARG, who + ": NULL context");

    // epochs in ascending order; the streams of an epoch keep their array order
    std::vector<u32> ep(n_streams);
    for (u32 i = 0; i < n_streams; i++) ep[i] = streams[i].epoch;
    std::sort(ep.begin(), ep.end()); ep.erase(std::unique(ep.begin(), ep.end()), ep.end());
    std::vector<PaEpoch> h_ep(ep.size());
    std::vector<std::vector<u32>> cnt_log(ep.size(), std::vector<u32>(32, 0));
    std::vector<PaStream> h_st(n_streams);
    std::vector<u32> h_tile(n_streams + 1, 0), h_base(n_streams + 1, 0);
    std::vector<const u32*> h_pay((size_t)n_streams * n_payload, nullptr);
    std::vector<u32*> h_prv((size_t)n_streams * n_payload, nullptr);
    for (u32 i = 0; i < n_streams; i++) {
        const nx_access_stream& s = streams[i];
        PaStream& d = h_st[i]; memset(&d, 0, sizeof d);
        const u32 slot = (u32)(std::lower_bound(ep.begin(), ep.end(), s.epoch) - ep.begin());
        const u64 n = (u64)1 << s.log_size;
        uintptr_t align = (uintptr_t)s.d_flag | (uintptr_t)s.d_ordinal;
        for (u32 c = 0; c < n_key_cols; c++) { d.key[c] = s.d_key[c]; align |= (uintptr_t)s.d_key[c]; }
        for (u32 c = 0; c < n_payload; c++) {
            h_pay[(size_t)i * n_payload + c] = s.d_payload ? s.d_payload[c] : nullptr;
            h_prv[(size_t)i * n_payload + c] = s.d_prev ? s.d_prev[c] : nullptr;
            align |= (uintptr_t)h_prv[(size_t)i * n_payload + c];
        }
        d.flag = s.d_flag; d.ord = s.d_ordinal; d.log_size = s.log_size; d.linear = s.linear != 0; d.epoch_slot = slot;
        d.vec = n >= 4 && !(align & 15);                          // aligned columns of whole quads: 16-byte loads and stores
        u32 ge = 0;                                               // earlier streams of the epoch with log_size >= L
        for (int L = 31; L >= 0; L--) { ge += cnt_log[slot][L]; d.before_ge[L] = (uint16_t)ge; }
        cnt_log[slot][s.log_size]++;
        h_tile[i + 1] = h_tile[i] + (u32)((n + PA_ENUM_TILE - 1) / PA_ENUM_TILE);
        h_base[i + 1] = h_base[i] + (u32)n;
    }
    u32 ebase = 0;
    for (size_t g = 0; g < ep.size(); g++) {
        PaEpoch& e = h_ep[g]; memset(&e, 0, sizeof e);
        e.base = ebase;
        for (u32 b = 0; b < 32; b++)
            for (u32 L = 0; L < 32; L++) { if (L >= b) e.ge[b] += cnt_log[g][L]; else e.small[b] += cnt_log[g][L] << L; }
        ebase += e.small[31] + (cnt_log[g][31] << 31);            // every stream has fewer than 2^31 rows
    }
    const u32 total = (u32)rows;
    const CountPlan plan = count_plan(rows);
    const u32 res_blocks = (total + PA_RES_TILE - 1) / PA_RES_TILE;
    const u32 n_pass = any_flag ? K.total_bits / 8 + 1 : (K.total_bits + 7) / 8;

    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_ctl = al(sizeof(PaCtl)), b_st = al(h_st.size() * sizeof(PaStream)), b_ep = al(h_ep.size() * sizeof(PaEpoch)), b_tile = al(h_tile.size() * 4),
                 b_base = al(h_base.size() * 4), b_ptr = al(h_pay.size() * sizeof(void*)), b_elems = al((size_t)total * 4), b_hist = al((size_t)plan.blocks * 256 * 4),
                 b_blk = al((size_t)res_blocks * 4);
    uint8_t* blob = nullptr;
    NX_TRY(dev_alloc(ctx, b_ctl + b_st + b_ep + b_tile + b_base + 2 * b_ptr + 4 * b_elems + b_hist + 2 * b_blk, (void**)&blob));
    uint8_t* at = blob;
    auto take = [&](size_t bytes) { uint8_t* p = at; at += bytes; return p; };
    PaCtl* d_ctl = (PaCtl*)take(b_ctl);
    PaStream* d_st = (PaStream*)take(b_st); PaEpoch* d_ep = (PaEpoch*)take(b_ep);
    u32* d_tile = (u32*)take(b_tile); u32* d_base = (u32*)take(b_base);
    const u32** d_pay = (const u32**)take(b_ptr); u32** d_prv = (u32**)take(b_ptr);
    u32* d_k[2]; u32* d_v[2];
    d_k[0] = (u32*)take(b_elems); d_v[0] = (u32*)take(b_elems); d_k[1] = (u32*)take(b_elems); d_v[1] = (u32*)take(b_elems);
    u32* d_hist = (u32*)take(b_hist); u32* d_cnt = (u32*)take(b_blk); u32* d_last = (u32*)take(b_blk);
    PaCtl h_ctl; memset(&h_ctl, 0, sizeof h_ctl); h_ctl.first_bad = ~(u64)0;
    int rc = upload_async_staged(ctx, d_ctl, &h_ctl, sizeof h_ctl);
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_st, h_st.data(), h_st.size() * sizeof(PaStream));
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_ep, h_ep.data(), h_ep.size() * sizeof(PaEpoch));
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_tile, h_tile.data(), h_tile.size() * 4);
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_base, h_base.data(), h_base.size() * 4);
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_pay, h_pay.data(), h_pay.size() * sizeof(void*));
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_prv, h_prv.data(), h_prv.size() * sizeof(void*));
    if (rc != NX_OK) { dev_free(ctx, blob); return rc; }

    hipLaunchKernelGGL(pa_enumerate_kernel, dim3(h_tile[n_streams]), dim3(PA_THREADS), 0, ctx->stream, (const PaStream*)d_st, (const PaEpoch*)d_ep, (const u32*)d_tile,
                       (const u32*)d_base, n_streams, K, n_payload, (u32* const*)d_prv, d_k[0], d_v[0], d_ctl);
    hipError_t e = hipGetLastError();
    u32 cur = 0;
    for (u32 p = 0; p < n_pass && e == hipSuccess; p++) {
        PaPass ps; ps.shift = 8 * p; ps.last = p + 1 == n_pass; ps.sentinel = std::min<u32>(255u, 1u << (K.total_bits - 8 * (n_pass - 1)));
        // (255 only without any d_flag and with whole-byte keys: PA_NONE is then a refused row alone, whose place does not matter)
        const PaSort sort = {d_k[cur], d_v[cur], d_k[cur ^ 1], d_v[cur ^ 1], ps};
        e = count_pass(ctx, sort, total, plan, 256, d_hist, nullptr, nullptr);
        cur ^= 1;
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pa_heads_kernel, dim3(res_blocks), dim3(PA_THREADS), 0, ctx->stream, (const u32*)d_k[cur], (const u32*)d_v[cur], total, d_cnt, d_last);
        hipLaunchKernelGGL(scan_kernel<0>, dim3(1), dim3(PA_THREADS), 0, ctx->stream, d_cnt, res_blocks, &d_ctl->n_keys);
        hipLaunchKernelGGL(scan_kernel<1>, dim3(1), dim3(PA_THREADS), 0, ctx->stream, d_last, res_blocks, (u32*)nullptr);
        hipLaunchKernelGGL(pa_resolve_kernel, dim3(res_blocks), dim3(PA_THREADS), 0, ctx->stream, (const u32*)d_k[cur], (const u32*)d_v[cur], total, (const u32*)d_cnt,
                           (const u32*)d_last, (const PaStream*)d_st, (const u32*)d_base, n_streams, n_payload, (const u32* const*)d_pay, (u32* const*)d_prv, h_init, h_sum);
        e = hipGetLastError();
    }
    if (e == hipSuccess) rc = copy_d2h_blocking(ctx, &h_ctl, d_ctl, sizeof h_ctl);
    // The copy above blocks, so every launch has completed.  Where a launch failed the copy is skipped and earlier kernels may still
    // run: the block then goes back to the context's cache, whose reuse is ordered on ctx->stream behind them.
    dev_free(ctx, blob);
    if (e != hipSuccess) return hip_fail(ctx, e, who.c_str(), __FILE__, __LINE__);
    if (rc != NX_OK) return rc;
    if (h_ctl.first_bad != ~(u64)0) {
        const u32 bs = (u32)(h_ctl.first_bad >> 32); const u64 bp = h_ctl.first_bad & 0xFFFFFFFFu;
        for (u32 c = 0; c < n_key_cols; c++) {                    // the row's k words, nothing else
            u32 x = 0;
            NX_TRY(copy_d2h_blocking(ctx, &x, streams[bs].d_key[c] + bp, 4));
            if (K.bits[c] < 32 && (x >> K.bits[c]))
                return set_err(ctx, NX_ERR_PROTOCOL, who + ": stream " + std::to_string(bs) + " row position " + std::to_string(bp) + ": key entry " + std::to_string(c) + " holds " +
                                                         std::to_string(x) + ", outside its " + std::to_string(K.bits[c]) + " bits");
        }
        return set_err(ctx, NX_ERR_PROTOCOL, who + ": stream " + std::to_string(bs) + " row position " + std::to_string(bp) + ": a key entry outside its bits");
    }
    if (n_keys) *n_keys = h_ctl.n_keys;
    return NX_OK;
}

}  // extern "C"
