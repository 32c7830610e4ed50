// Lookup multiplicities for a table that is a SPARSE subset of a key space of up to 32 bits: the boundary tables keyed by an address.
//
// nx_logup_multiplicities (multiplicity.hip) keeps one counter per key of the key space, which is right for the range and bitwise
// tables and impossible for the reference's address-keyed tables: prover2's PrivateMemoryBoundary has one row per touched RAM address
// with MultiplicityRead / MultiplicityWrite from the AddressAccessSideNote (read_write_memory_boundary/private_memory/mod.rs:95-168,
// 249-262), its Pub / Static / ProgramMemoryBoundary and v1's FinalPrgMemoryCtr are keyed the same way.  Here the counters belong to
// the table's rows, and a looked-up row finds its counter by a search:
//   index    the valid table rows become (key, position) pairs sorted by key: ceil(sum of key_bits / 8) passes of the counting pass of
//            count_pass.cuh with the policy MsSort, whose first pass reads the table columns themselves (a row that is no table row is
//            no element, so the pairs leave it packed) and whose later passes move the pairs.  One pass over neighbours (check) then
//            finds two rows with one key and, back at the rows, an entry outside its bits.
//   count    one launch for all uses, tiled like mult_count_kernel.  A key is searched in two levels: every 2^log_stride-th sorted key
//            is a splitter, staged once per block in LDS (a table of up to MS_LDS_KEYS rows is staged whole), the segment behind the
//            splitter is searched in global memory; both are fixed-trip binary searches, the 16 rows of a lane side by side.  The
//            splitters are gathered once into a packed array (ms_split_kernel), so a block stages them with consecutive loads.  Equal
//            results are merged before they reach a counter (runs inside a lane; one add for a wave that holds one key), the add is a
//            64-bit global atomic into counter[sorted index].  A row that finds nothing adds to the missing weight instead.
//   scatter  d_mult[position[i]] = counter[i] mod p; a row that is no table row gets 0.
//   missing  only when the missing weight is not zero or a row held an entry outside its bits: the same walk counts those rows and
//            finds the smallest (use << 32 | position).
// Only integer sums and minima cross lanes and blocks; blocks meet at kernel boundaries only.  The tile walk and the tile load are
// those of multiplicity.hip restated (that file's lines are cited by number elsewhere and stay where they are), with the one change a
// 32-bit entry needs: no shift by 32.
#include "internal.h"
#include <algorithm>
#include <string.h>
#include <string>

namespace nx {

#include "count_pass.cuh"

#ifndef NX_MULT_SPARSE_LDS_LOG_KEYS
#error "include/nexus_hip.h defines NX_MULT_SPARSE_LDS_LOG_KEYS"
#endif
static_assert(NX_MULT_SPARSE_LDS_LOG_KEYS >= 1 && NX_MULT_SPARSE_LDS_LOG_KEYS <= 13, "1 to 13: two splitters at least, 32 KiB of LDS at most");
constexpr u32 MS_QUADS = 4, MS_THREADS = CP_THREADS, MS_TILE = MS_THREADS * MS_QUADS * 4;   // rows a block takes per step
constexpr u32 MS_LDS_LOG_KEYS = NX_MULT_SPARSE_LDS_LOG_KEYS, MS_LDS_KEYS = 1u << MS_LDS_LOG_KEYS;   // a table of more rows is searched in two levels
constexpr u32 MS_MAX_USES = 1u << 16;
// The scan of a counting pass is ONE block over 256 words per block of the pass, and a table is sorted in up to four passes: with the
// 1024 blocks count_plan gives 2^20 rows the four scans took 0.76 ms of a 1.28 ms call.  A block of this sort takes more tiles instead.
constexpr u32 MS_SORT_BLOCKS = 256;
static inline CountPlan ms_count_plan(u64 total) {
    const u64 per = (u64)CP_THREADS * std::min<u32>(CP_MAX_BLOCKS, MS_SORT_BLOCKS);
    CountPlan p;
    p.tiles = std::max<u32>(CP_MIN_TILES, (u32)((total + per - 1) / per));
    p.blocks = (u32)((total + (u64)p.tiles * CP_THREADS - 1) / ((u64)p.tiles * CP_THREADS));
    return p;
}

struct MsUse { const u32* col[4]; const u32* weight; u32 log_size, vec; };
struct MsTable { const u32* col[4]; const u32* valid; };
// results and flags of one call, one 64-byte block of device memory
struct MsCtl {
    u64 missing_weight;  // weight of the rows that found no table row
    u64 n_missing;
    u64 first_missing;   // min (use << 32 | position), ~0 = none
    u64 tab_dup;         // min (position << 32 | first position with the same key) over the second rows of a key, ~0 = none
    u32 row_oor;         // some counted row held an entry >= 2^key_bits
    u32 tab_oor_pos;     // min position of a valid table row with such an entry, ~0 = none
    u32 n_valid;         // table rows = elements of the index
    u32 pad[5];
};
static_assert(sizeof(MsCtl) == 64, "one 64-byte block");

__device__ __forceinline__ u64 ms_wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void ms_pack(const u32* const col[4], const PackedKey& K, u32 row, u32* key, u32* out) {
    u32 k = 0, o = 0;
#pragma unroll
    for (u32 c = 0; c < 4; c++)
        if (c < K.n_cols) { const u32 x = gld(col[c] + row); k |= x << K.shift[c]; o |= K.bits[c] < 32 ? x >> K.bits[c] : 0u; }
    *key = k; *out = o;
}

// One pass of the index sort as a counting pass.  first: element j is table row j where it is a table row, its digit comes from the
// packed key; later passes read the pairs the pass before left packed, *n_valid of them.
struct MsSort {
    MsTable t; PackedKey K;
    const u32* kin; const u32* vin; u32* kout; u32* vout; const u32* n_valid;
    u32 shift, first;
    struct Item { u32 key, val; };
    __device__ __forceinline__ bool load(u32 j, u32 total, Item* it, u32* d) const {
        bool have;
        it->key = 0; it->val = 0;
        if (first) {
            have = j < total && (!t.valid || gld(t.valid + j) != 0);
            if (have) { u32 out; ms_pack(t.col, K, j, &it->key, &out); it->val = j; }
        } else {
            have = j < total && j < gld(n_valid);
            if (have) { it->key = gld(kin + j); it->val = gld(vin + j); }
        }
        *d = have ? (it->key >> shift) & 255u : 0u;
        return have;
    }
    __device__ __forceinline__ bool digit(u32 j, u32 total, u32* d) const {
        bool have; u32 key = 0;
        if (first) {
            have = j < total && (!t.valid || gld(t.valid + j) != 0);
            if (have) { u32 out; ms_pack(t.col, K, j, &key, &out); }
        } else {
            have = j < total && j < gld(n_valid);
            if (have) key = gld(kin + j);
        }
        *d = have ? (key >> shift) & 255u : 0u;
        return have;
    }
    __device__ __forceinline__ void store(u32 slot, const Item& it) const { gst(kout + slot, it.key); gst(vout + slot, it.val); }
};

// sorted pair i: an entry of its row outside its bits; the second row of a key (positions ascend inside a key: the sort is stable)
__global__ __launch_bounds__(MS_THREADS) void ms_check_kernel(const u32* __restrict__ keys, const u32* __restrict__ pos, MsTable t, PackedKey K, MsCtl* __restrict__ ctl) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gld(&ctl->n_valid)) return;
    const u32 k = gld(keys + i), p = gld(pos + i);
    u32 again, out;
    ms_pack(t.col, K, p, &again, &out);
    if (out) atomicMin(&ctl->tab_oor_pos, p);
    if (i > 0 && gld(keys + i - 1) == k && (i < 2 || gld(keys + i - 2) != k))
        atomicMin((unsigned long long*)&ctl->tab_dup, ((unsigned long long)p << 32) | gld(pos + i - 1));
}

// The 16 rows of this lane in the tile at `row0` of use `u`: row (q, e) is row0 + (q * 256 + lane) * 4 + e.  key: the packed key;
// wt: the numerator (1 without a weight column), 0 for a row past the end, a weight-0 row and — with its bit set in *bad — a row
// that has a nonzero weight and an entry outside its key_bits.
__device__ __forceinline__ void ms_load_tile(const MsUse& u, const PackedKey& K, u32 row0, u32 key[16], u32 wt[16], u32* bad) {
    const u32 n = 1u << u.log_size;
    const bool vec = u.vec != 0;
    uint4 v[4][MS_QUADS], w[MS_QUADS];
#pragma unroll
    for (u32 c = 0; c < 4; c++)
        if (c < K.n_cols) {
#pragma unroll
            for (u32 q = 0; q < MS_QUADS; q++) v[c][q] = gld4_guarded(u.col[c], row0 + (q * MS_THREADS + threadIdx.x) * 4, n, vec);
        }
#pragma unroll
    for (u32 q = 0; q < MS_QUADS; q++) {
        const u32 r = row0 + (q * MS_THREADS + threadIdx.x) * 4;
        if (u.weight) w[q] = gld4_guarded(u.weight, r, n, vec);
        else w[q] = make_uint4(r < n, r + 1 < n, r + 2 < n, r + 3 < n);
    }
    u32 b = 0;
#pragma unroll
    for (u32 q = 0; q < MS_QUADS; q++) {
        u32 k[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
#pragma unroll
        for (u32 c = 0; c < 4; c++)
            if (c < K.n_cols) {
                const u32 x[4] = {v[c][q].x, v[c][q].y, v[c][q].z, v[c][q].w};
#pragma unroll
                for (u32 e = 0; e < 4; e++) { k[e] |= x[e] << K.shift[c]; o[e] |= K.bits[c] < 32 ? x[e] >> K.bits[c] : 0u; }
            }
        const u32 ww[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
#pragma unroll
        for (u32 e = 0; e < 4; e++) {
            const bool out = o[e] != 0 && ww[e] != 0;
            if (out) b |= 1u << (4 * q + e);
            key[4 * q + e] = out ? 0u : k[e];
            wt[4 * q + e] = out ? 0u : ww[e];
        }
    }
    *bad = b;
}

// The tiles of all uses form one sequence (tile_start: first tile of every use, n_uses + 1 entries); a block takes a contiguous part
// of it, so it looks its first use up once and then only steps forward.
struct MsWalk {
    const MsUse* uses; const u32* tile_start; u32 n_uses, tile, tile_end, use;
    __device__ void begin(const MsUse* us, const u32* ts, u32 n) {
        uses = us; tile_start = ts; n_uses = n;
        const u64 total = ts[n];
        tile = (u32)(total * blockIdx.x / gridDim.x); tile_end = (u32)(total * (blockIdx.x + 1) / gridDim.x);
        use = find_le(ts, n, tile);
    }
    __device__ bool next(MsUse* u, u32* row0) {
        if (tile >= tile_end) return false;
        while (tile >= tile_start[use + 1]) use++;
        *u = uses[use];
        *row0 = (tile - tile_start[use]) * MS_TILE;
        tile++;
        return true;
    }
};

// splits[s] = keys[s << log_stride]: the splitters next to each other, so that every block of the walks stages them with consecutive
// loads (gathered by every block they would cost one cache line per splitter and block)
__global__ __launch_bounds__(MS_THREADS) void ms_split_kernel(const u32* __restrict__ keys, u32 log_stride, const MsCtl* __restrict__ ctl, u32* __restrict__ splits) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x, n = gld(&ctl->n_valid);
    if (((u64)s << log_stride) < n) gst(splits + s, gld(keys + ((size_t)s << log_stride)));
}

// The index as a block sees it: split[s] = keys[s << log_stride] for the ns splitters (in LDS), keys[0 .. n) ascending in global memory.
struct MsIndex { const u32* split; const u32* keys; u32 n, ns, top, log_stride; };

// stages the splitters; every thread of the block calls it, a barrier follows inside
__device__ __forceinline__ MsIndex ms_index_begin(u32* split, const u32* __restrict__ splits, const u32* __restrict__ keys, u32 n, u32 log_stride) {
    MsIndex X;
    X.split = split; X.keys = keys; X.n = n; X.log_stride = log_stride;
    X.ns = (u32)(((u64)n + (1u << log_stride) - 1) >> log_stride);
    X.top = X.ns > 1 ? 1u << (31 - __builtin_clz(X.ns - 1)) : 0u;      // the largest power of two below ns
    for (u32 s = threadIdx.x; s < X.ns; s += MS_THREADS) split[s] = gld(splits + s);
    __syncthreads();
    return X;
}

// N keys side by side: idx[i] = the last sorted index whose key is <= key[i] (0 when there is none); bit i of the result: that key IS
// key[i].  Both levels make a fixed number of steps, the same for every lane; an index past the end is clamped for the load and never taken.
template <int N> __device__ __forceinline__ u32 ms_search(const MsIndex& X, const u32* key, u32* idx) {
    if (X.n == 0) {
#pragma unroll
        for (int i = 0; i < N; i++) idx[i] = 0;
        return 0;
    }
    u32 lo[N], val[N];
    const u32 v0 = X.split[0];
#pragma unroll
    for (int i = 0; i < N; i++) { lo[i] = 0; val[i] = v0; }
    for (u32 h = X.top; h; h >>= 1) {
#pragma unroll
        for (int i = 0; i < N; i++) {
            const u32 m = lo[i] + h, v = X.split[min(m, X.ns - 1)];
            const bool take = m < X.ns && v <= key[i];
            lo[i] = take ? m : lo[i]; val[i] = take ? v : val[i];
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) lo[i] <<= X.log_stride;
    for (u32 h = (1u << X.log_stride) >> 1; h; h >>= 1) {
        u32 v[N];
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = gld(X.keys + min(lo[i] + h, X.n - 1));      // all loads of a step before the first compare
#pragma unroll
        for (int i = 0; i < N; i++) {
            const u32 m = lo[i] + h;
            const bool take = m < X.n && v[i] <= key[i];
            lo[i] = take ? m : lo[i]; val[i] = take ? v[i] : val[i];
        }
    }
    u32 found = 0;
#pragma unroll
    for (int i = 0; i < N; i++) { idx[i] = lo[i]; found |= (u32)(val[i] == key[i]) << i; }
    return found;
}

__global__ __launch_bounds__(MS_THREADS) void ms_count_kernel(const MsUse* __restrict__ uses, const u32* __restrict__ tile_start, u32 n_uses, PackedKey K,
                                                              const u32* __restrict__ splits, const u32* __restrict__ skeys, u32 log_stride, u64* __restrict__ counters,
                                                              MsCtl* __restrict__ ctl) {
    __shared__ u32 split[MS_LDS_KEYS];
    const MsIndex X = ms_index_begin(split, splits, skeys, gld(&ctl->n_valid), log_stride);
    auto add = [&](u32 i, u64 amount) { atomicAdd((unsigned long long*)&counters[i], (unsigned long long)amount); };
    MsWalk walk; walk.begin(uses, tile_start, n_uses);
    MsUse u; u32 row0;
    bool any_bad = false;
    u64 miss = 0;
    while (walk.next(&u, &row0)) {                            // uniform over the block
        u32 key[16], wt[16], bad;
        ms_load_tile(u, K, row0, key, wt, &bad);
        any_bad |= bad != 0;
        // one key in the whole lane?
        u64 total = 0; u32 k0 = 0; bool single = true;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (wt[i]) { if (total && key[i] != k0) single = false; if (!total) k0 = key[i]; total += wt[i]; }
        }
        const u64 holders = __ballot(total != 0);
        if (holders == 0) continue;                           // uniform over the wave
        const int leader = __ffsll((unsigned long long)holders) - 1;
        const u32 kl = __shfl(k0, leader, 64);
        if (__all(single && (total == 0 || k0 == kl))) {      // one key in the whole wave: one search, one add
            const u64 s = ms_wave_sum(total);
            u32 at;
            const u32 hit = ms_search<1>(X, &kl, &at);
            if ((int)(threadIdx.x & 63) == leader) { if (hit) add(at, s); else miss += s; }
            continue;
        }
        u32 idx[16];
        const u32 hit = ms_search<16>(X, key, idx);
        u64 acc = 0; u32 cur = 0;                             // runs of equal results
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (!wt[i]) continue;
            if (!((hit >> i) & 1)) { miss += wt[i]; continue; }
            if (acc && idx[i] != cur) { add(cur, acc); acc = 0; }
            cur = idx[i]; acc += wt[i];
        }
        if (acc) add(cur, acc);
    }
    if (any_bad) gst(&ctl->row_oor, 1u);
    miss = ms_wave_sum(miss);
    if ((threadIdx.x & 63) == 0 && miss) atomicAdd((unsigned long long*)&ctl->missing_weight, (unsigned long long)miss);
}

// thread j: row j gets 0 when it is no table row; sorted pair j puts its counter at its row
__global__ __launch_bounds__(MS_THREADS) void ms_scatter_kernel(const u32* __restrict__ pos, const u64* __restrict__ counters, const u32* __restrict__ valid, u32 n_rows,
                                                                u32* __restrict__ d_mult, const MsCtl* __restrict__ ctl) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    if (valid && gld(valid + j) == 0) gst(d_mult + j, 0u);
    if (j < gld(&ctl->n_valid)) gst(d_mult + gld(pos + j), (u32)(counters[j] % P));
}

// a counted row is missing when its key is no key of the index
__global__ __launch_bounds__(MS_THREADS) void ms_missing_kernel(const MsUse* __restrict__ uses, const u32* __restrict__ tile_start, u32 n_uses, PackedKey K,
                                                                const u32* __restrict__ splits, const u32* __restrict__ skeys, u32 log_stride, MsCtl* __restrict__ ctl) {
    __shared__ u32 split[MS_LDS_KEYS];
    const MsIndex X = ms_index_begin(split, splits, skeys, gld(&ctl->n_valid), log_stride);
    MsWalk walk; walk.begin(uses, tile_start, n_uses);
    MsUse u; u32 row0;
    u64 n = 0, first = ~(u64)0;
    while (walk.next(&u, &row0)) {
        const u32 use = walk.use;
        u32 key[16], wt[16], idx[16], bad;
        ms_load_tile(u, K, row0, key, wt, &bad);
        const u32 hit = ms_search<16>(X, key, idx);
#pragma unroll
        for (u32 i = 0; i < 16; i++) {
            const bool miss = ((bad >> i) & 1) || (wt[i] && !((hit >> i) & 1));
            if (miss) {
                const u64 at = ((u64)use << 32) | (row0 + ((i >> 2) * MS_THREADS + threadIdx.x) * 4 + (i & 3));
                n++; first = at < first ? at : first;
            }
        }
    }
    if (n) { atomicAdd((unsigned long long*)&ctl->n_missing, (unsigned long long)n); atomicMin((unsigned long long*)&ctl->first_missing, (unsigned long long)first); }
}

}  // namespace nx

using namespace nx;

extern "C" {

int nx_logup_multiplicities_sparse(nx_ctx* ctx, const nx_lookup_use* uses, uint32_t n_uses, uint32_t n_key_cols, const uint32_t* key_bits,
                                   const uint32_t* const* d_table, const uint32_t* d_table_valid, uint32_t log_table, uint32_t* d_mult,
                                   uint64_t* n_missing, uint32_t* first_missing_use, uint64_t* first_missing_pos) {
    NX_GUARD(ctx);
    const std::string who = "nx_logup_multiplicities_sparse";
    if (!ctx || !key_bits || !d_table || !d_mult || (n_uses && !uses)) return set_err(ctx, NX_ERR_ARG, who + ": NULL argument");
    if (n_key_cols < 1 || n_key_cols > 4) return set_err(ctx, NX_ERR_ARG, who + ": 1 to 4 key columns");
    PackedKey K; memset(&K, 0, sizeof K);
    K.n_cols = n_key_cols;
    for (u32 c = 0; c < n_key_cols; c++) {
        if (key_bits[c] < 1 || key_bits[c] > 32) return set_err(ctx, NX_ERR_ARG, who + ": key_bits of 1 to 32 per column");
        K.bits[c] = key_bits[c]; K.shift[c] = K.total_bits; K.total_bits += key_bits[c];
        if (K.total_bits > 32) return set_err(ctx, NX_ERR_ARG, who + ": the key_bits add up to more than 32");
    }
    if (log_table > 30) return set_err(ctx, NX_ERR_ARG, who + ": log_table of " + std::to_string(log_table) + ", 0 to 30");
    if (n_uses > MS_MAX_USES) return set_err(ctx, NX_ERR_ARG, who + ": at most 65536 uses per call");
    MsTable table; memset(&table, 0, sizeof table);
    table.valid = d_table_valid;
    bool alias = d_table_valid == d_mult;
    for (u32 c = 0; c < n_key_cols; c++) {
        if (!d_table[c]) return set_err(ctx, NX_ERR_ARG, who + ": NULL table column");
        table.col[c] = d_table[c]; alias |= d_table[c] == d_mult;
    }
    std::vector<MsUse> h_uses(std::max<u32>(1, n_uses));
    std::vector<u32> h_start(n_uses + 1, 0);
    u64 rows = 0;
    for (u32 i = 0; i < n_uses; i++) {
        const nx_lookup_use& s = uses[i];
        if (s.log_size > 30) return set_err(ctx, NX_ERR_ARG, who + ": use " + std::to_string(i) + ": log_size too large");
        rows += (u64)1 << s.log_size;
        if (rows > ((u64)1 << 32)) return set_err(ctx, NX_ERR_ARG, who + ": more than 2^32 rows in one call");
        if (!s.d_values) return set_err(ctx, NX_ERR_ARG, who + ": use " + std::to_string(i) + ": NULL d_values");
        MsUse& u = h_uses[i]; memset(&u, 0, sizeof u);
        const u64 n = (u64)1 << s.log_size;
        uintptr_t align = (uintptr_t)s.d_weight;
        alias |= s.d_weight == d_mult;
        for (u32 c = 0; c < n_key_cols; c++) {
            if (!s.d_values[c]) return set_err(ctx, NX_ERR_ARG, who + ": use " + std::to_string(i) + ": NULL value column");
            u.col[c] = s.d_values[c]; align |= (uintptr_t)s.d_values[c]; alias |= s.d_values[c] == d_mult;
        }
        u.weight = s.d_weight; u.log_size = s.log_size;
        u.vec = n >= MS_TILE && !(align & 15);                // whole tiles of aligned columns: 16-byte loads
        h_start[i + 1] = h_start[i] + (u32)((n + MS_TILE - 1) / MS_TILE);
    }
    if (alias) return set_err(ctx, NX_ERR_ARG, who + ": d_mult has the pointer of an input column of the call");
    const u32 n_tiles = h_start[n_uses], n_rows = 1u << log_table;
    const CountPlan plan = ms_count_plan(n_rows);
    const u32 n_pass = (K.total_bits + 7) / 8;
    const u32 log_stride = log_table > MS_LDS_LOG_KEYS ? log_table - MS_LDS_LOG_KEYS : 0u;   // a table of up to MS_LDS_KEYS rows is staged whole

    // one block: the control words, the use table, the tile starts, two (key, position) buffers, the digit counts, the packed splitters
    // (a table the LDS holds whole is its own splitter array).  The counters take the pair buffer the last sort pass has read: 8 bytes per row.
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_ctl = al(sizeof(MsCtl)), b_uses = al(h_uses.size() * sizeof(MsUse)), b_start = al(h_start.size() * 4), b_elems = al((size_t)n_rows * 4),
                 b_hist = al((size_t)plan.blocks * 256 * 4), b_split = log_stride ? al((size_t)MS_LDS_KEYS * 4) : 0;
    uint8_t* blob = nullptr;
    NX_TRY(dev_alloc(ctx, b_ctl + b_uses + b_start + 4 * b_elems + b_hist + b_split, (void**)&blob));
    uint8_t* at = blob;
    auto take = [&](size_t bytes) { uint8_t* p = at; at += bytes; return p; };
    MsCtl* d_ctl = (MsCtl*)take(b_ctl);
    const MsUse* d_uses = (const MsUse*)take(b_uses); const u32* d_start = (const u32*)take(b_start);
    u32* d_k[2]; u32* d_v[2];
    d_k[0] = (u32*)take(b_elems); d_v[0] = (u32*)take(b_elems); d_k[1] = (u32*)take(b_elems); d_v[1] = (u32*)take(b_elems);
    u32* d_hist = (u32*)take(b_hist); u32* d_split = (u32*)take(b_split);
    MsCtl h_ctl; memset(&h_ctl, 0, sizeof h_ctl);
    h_ctl.first_missing = ~(u64)0; h_ctl.tab_dup = ~(u64)0; h_ctl.tab_oor_pos = ~0u;
    int rc = upload_async_staged(ctx, d_ctl, &h_ctl, sizeof h_ctl);
    if (rc == NX_OK) rc = upload_async_staged(ctx, (void*)d_uses, h_uses.data(), h_uses.size() * sizeof(MsUse));
    if (rc == NX_OK) rc = upload_async_staged(ctx, (void*)d_start, h_start.data(), h_start.size() * 4);
    if (rc != NX_OK) { dev_free(ctx, blob); return rc; }

    hipError_t e = hipSuccess;
    u32 cur = 1;                                              // the first pass reads the table and fills buffer 0
    for (u32 p = 0; p < n_pass && e == hipSuccess; p++) {
        MsSort sort; memset(&sort, 0, sizeof sort);
        sort.t = table; sort.K = K; sort.kin = d_k[cur]; sort.vin = d_v[cur]; sort.kout = d_k[cur ^ 1]; sort.vout = d_v[cur ^ 1];
        sort.n_valid = &d_ctl->n_valid; sort.shift = 8 * p; sort.first = p == 0;
        e = count_pass(ctx, sort, n_rows, plan, 256, d_hist, p == 0 ? &d_ctl->n_valid : nullptr, nullptr);
        cur ^= 1;
    }
    u64* d_cnt = (u64*)d_k[cur ^ 1];                          // d_k[x] and d_v[x] are adjacent: 8 bytes per row
    const u32 row_grid = (n_rows + MS_THREADS - 1) / MS_THREADS;
    const u32 walk_grid = std::max<u32>(1, std::min<u32>(n_tiles, (u32)ctx->n_cus * 4));
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (size_t)n_rows * 8, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ms_check_kernel, dim3(row_grid), dim3(MS_THREADS), 0, ctx->stream, (const u32*)d_k[cur], (const u32*)d_v[cur], table, K, d_ctl);
        if (!log_stride) d_split = d_k[cur];
        else if (n_tiles) hipLaunchKernelGGL(ms_split_kernel, dim3((MS_LDS_KEYS + MS_THREADS - 1) / MS_THREADS), dim3(MS_THREADS), 0, ctx->stream, (const u32*)d_k[cur], log_stride,
                                              (const MsCtl*)d_ctl, d_split);
        if (n_tiles)
            hipLaunchKernelGGL(ms_count_kernel, dim3(walk_grid), dim3(MS_THREADS), 0, ctx->stream, d_uses, d_start, n_uses, K, (const u32*)d_split, (const u32*)d_k[cur], log_stride, d_cnt,
                               d_ctl);
        hipLaunchKernelGGL(ms_scatter_kernel, dim3(row_grid), dim3(MS_THREADS), 0, ctx->stream, (const u32*)d_v[cur], (const u64*)d_cnt, d_table_valid, n_rows, d_mult,
                           (const MsCtl*)d_ctl);
        e = hipGetLastError();
    }
    if (e == hipSuccess) rc = copy_d2h_blocking(ctx, &h_ctl, d_ctl, sizeof h_ctl);
    if (e == hipSuccess && rc == NX_OK && h_ctl.tab_oor_pos == ~0u && h_ctl.tab_dup == ~(u64)0 && (h_ctl.missing_weight || h_ctl.row_oor) && n_tiles) {
        hipLaunchKernelGGL(ms_missing_kernel, dim3(walk_grid), dim3(MS_THREADS), 0, ctx->stream, d_uses, d_start, n_uses, K, (const u32*)d_split, (const u32*)d_k[cur], log_stride, d_ctl);
        e = hipGetLastError();
        if (e == hipSuccess) rc = copy_d2h_blocking(ctx, &h_ctl, d_ctl, sizeof h_ctl);
    }
    // The copies above block, so every launch has completed.  Where a launch failed they are skipped and earlier kernels may still
    // run: the block then goes back to the context's cache, whose reuse is ordered on ctx->stream behind them.
    dev_free(ctx, blob);
    if (e != hipSuccess) return hip_fail(ctx, e, who.c_str(), __FILE__, __LINE__);
    if (rc != NX_OK) return rc;
    if (h_ctl.tab_oor_pos != ~0u)
        return set_err(ctx, NX_ERR_ARG, who + ": table row position " + std::to_string(h_ctl.tab_oor_pos) + " holds a value outside its key_bits");
    if (h_ctl.tab_dup != ~(u64)0) {
        const u32 p1 = (u32)(h_ctl.tab_dup >> 32), p0 = (u32)h_ctl.tab_dup;
        std::string t;
        for (u32 c = 0; c < n_key_cols; c++) {
            u32 x = 0;
            NX_TRY(copy_d2h_blocking(ctx, &x, d_table[c] + p1, 4));
            t += (c ? ", " : "") + std::to_string(x);
        }
        return set_err(ctx, NX_ERR_ARG, who + ": table row positions " + std::to_string(p0) + " and " + std::to_string(p1) + " hold the same key (" + t + ")");
    }
    if (n_missing) *n_missing = h_ctl.n_missing;
    if (first_missing_use) *first_missing_use = h_ctl.n_missing ? (u32)(h_ctl.first_missing >> 32) : 0;
    if (first_missing_pos) *first_missing_pos = h_ctl.n_missing ? (h_ctl.first_missing & 0xFFFFFFFFu) : 0;
    if (!h_ctl.n_missing) return NX_OK;
    const u32 mu = (u32)(h_ctl.first_missing >> 32); const u64 mp = h_ctl.first_missing & 0xFFFFFFFFu;
    std::string t;
    for (u32 c = 0; c < n_key_cols; c++) {                    // the row's k words, nothing else
        u32 x = 0;
        NX_TRY(copy_d2h_blocking(ctx, &x, uses[mu].d_values[c] + mp, 4));
        t += (c ? ", " : "") + std::to_string(x);
    }
    return set_err(ctx, NX_ERR_PROTOCOL, who + ": use " + std::to_string(mu) + " row position " + std::to_string(mp) + ": (" + t + ") is not a row of the table (" +
                                             std::to_string(h_ctl.n_missing) + " such row" + (h_ctl.n_missing == 1 ? "" : "s") + ")");
}

}  // extern "C"
