// Lookup multiplicities on the device: the TABLE side of a logup argument.
//
// The reference counts on the CPU how often every row of a lookup table was used: the v1 `Multiplicity<LEN, L>` extensions
// (prover/src/extensions/multiplicity.rs:143-237), the bitwise tables and prover2's range_multiplicity / bitwise_multiplicity
// components take their one main-trace column from the `SideNote`.  Without that column the claimed sums of a proof do not cancel and
// the verifier refuses it (prover/src/machine.rs:343; prover2/machine/src/verify.rs:145-160).  Here the count is a histogram over
// columns that already live in HBM:
//   count    every use (k key columns + an optional numerator column, any row order) is walked once, 16 B per lane and load; the key
//            of a row is the concatenation of its entries.  Key spaces of <= 2^NX_MULT_LDS_MAX_KEY_BITS keys are counted in
//            block-private LDS counters and flushed with one global atomic per nonzero counter and block; wider ones go straight to
//            the 2^(sum of key_bits) global counters.  All counters are 64-bit integers: the sums are exact and the same on every run.
//   scatter  table position pos packs its key, takes the counter (exchange with a sentinel: a second taker is a duplicate key) and
//            writes counter mod p.
//   residual what is left in counters nobody took is the weight of rows that are in no table row.
//   missing  only when that weight is not zero or a row held an entry outside its key_bits: counts those rows and finds the smallest
//            (use << 32 | position).
// Byte-limb traces are skewed (whole columns are zero), so equal keys are combined before they reach a counter: a lane merges runs
// of equal keys among its 16 rows, a wave whose lanes all hold one key adds once, and the LDS counters are replicated (one copy per
// lane residue, copies an odd number of words apart so that the same key in different copies falls into different banks).
#include "internal.h"
#include <algorithm>
#include <string.h>
#include <string>

namespace nx {

constexpr u32 MULT_QUADS = 4, MULT_THREADS = 256, MULT_TILE = MULT_THREADS * MULT_QUADS * 4;   // rows a block takes per step
constexpr u32 MULT_LDS_KEYS = 1u << NX_MULT_LDS_MAX_KEY_BITS, MULT_LDS_COPIES = 32, MULT_LDS_WORDS = MULT_LDS_KEYS + MULT_LDS_COPIES;
constexpr u64 MULT_TAKEN = ~(u64)0;            // a counter the scatter pass has taken; no sum reaches it (< 2^32 rows * p)
constexpr u32 MULT_MAX_USES = 1u << 16;

struct MultUse { const u32* col[4]; const u32* weight; u32 log_size, vec; };
// results and flags of one call, one 64-byte block of device memory
struct MultCtl {
    u64 residual;        // weight counted on keys no table row has
    u64 n_missing;
    u64 first_missing;   // min (use << 32 | position), ~0 = none
    u32 row_oor;         // some counted row held an entry >= 2^key_bits
    u32 tab_oor_pos;     // min position of a table row with such an entry, ~0 = none
    u32 tab_dup_key;     // min key two table rows share, ~0 = none
    u32 pad[7];
};

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The 16 rows of this lane in the tile at `row0` of use `u`: row (q, e) is row0 + (q * 256 + lane) * 4 + e.  key: the packed key;
// wt: the numerator (1 without a weight column), 0 for a row past the end, a weight-0 row and — with its bit set in *bad — a row
// that has a nonzero weight and an entry outside its key_bits.
__device__ __forceinline__ void mult_load_tile(const MultUse& u, const PackedKey& K, u32 row0, u32 key[16], u32 wt[16], u32* bad) {
    const u32 n = 1u << u.log_size;
    const bool vec = u.vec != 0;
    uint4 v[4][MULT_QUADS], w[MULT_QUADS];
#pragma unroll
    for (u32 c = 0; c < 4; c++)
        if (c < K.n_cols) {
#pragma unroll
            for (u32 q = 0; q < MULT_QUADS; q++) v[c][q] = gld4_guarded(u.col[c], row0 + (q * MULT_THREADS + threadIdx.x) * 4, n, vec);
        }
#pragma unroll
    for (u32 q = 0; q < MULT_QUADS; q++) {
        const u32 r = row0 + (q * MULT_THREADS + threadIdx.x) * 4;
        if (u.weight) w[q] = gld4_guarded(u.weight, r, n, vec);
        else w[q] = make_uint4(r < n, r + 1 < n, r + 2 < n, r + 3 < n);
    }
    u32 b = 0;
#pragma unroll
    for (u32 q = 0; q < MULT_QUADS; q++) {
        u32 k[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
#pragma unroll
        for (u32 c = 0; c < 4; c++)
            if (c < K.n_cols) {
                const u32 x[4] = {v[c][q].x, v[c][q].y, v[c][q].z, v[c][q].w};
#pragma unroll
                for (u32 e = 0; e < 4; e++) { k[e] |= x[e] << K.shift[c]; o[e] |= x[e] >> K.bits[c]; }
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
struct MultWalk {
    const MultUse* uses; const u32* tile_start; u32 n_uses, tile, tile_end, use;
    __device__ void begin(const MultUse* us, const u32* ts, u32 n) {
        uses = us; tile_start = ts; n_uses = n;
        const u64 total = ts[n];
        tile = (u32)(total * blockIdx.x / gridDim.x); tile_end = (u32)(total * (blockIdx.x + 1) / gridDim.x);
        u32 lo = 0, hi = n;                                   // the last use with tile_start <= tile
        while (hi - lo > 1) { const u32 mid = (lo + hi) / 2; if (ts[mid] <= tile) lo = mid; else hi = mid; }
        use = lo;
    }
    __device__ bool next(MultUse* u, u32* row0) {
        if (tile >= tile_end) return false;
        while (tile >= tile_start[use + 1]) use++;
        *u = uses[use];
        *row0 = (tile - tile_start[use]) * MULT_TILE;
        tile++;
        return true;
    }
};

// LDS: block-private counters, flushed at the end.  !LDS: every add goes to the global counters.
template <bool LDS>
__global__ __launch_bounds__(MULT_THREADS) void mult_count_kernel(const MultUse* __restrict__ uses, const u32* __restrict__ tile_start, u32 n_uses, PackedKey K,
                                                                  u64* __restrict__ counters, MultCtl* __restrict__ ctl) {
    __shared__ u64 lds[LDS ? MULT_LDS_WORDS : 1];
    const u32 n_keys = 1u << K.total_bits;
    // copies of the counters: as many as fit, at most 32; copy c starts at c * (n_keys + 1)
    const u32 copies = LDS ? min(MULT_LDS_COPIES, MULT_LDS_KEYS >> K.total_bits) : 1u;
    const u32 my_copy = (threadIdx.x & (copies - 1)) * (n_keys + 1);
    if (LDS) {
        for (u32 i = threadIdx.x; i < copies * (n_keys + 1); i += MULT_THREADS) lds[i] = 0;
        __syncthreads();
    }
    auto add = [&](u32 key, u64 amount) {
        if (LDS) atomicAdd((unsigned long long*)&lds[my_copy + key], (unsigned long long)amount);
        else atomicAdd((unsigned long long*)&counters[key], (unsigned long long)amount);
    };
    MultWalk walk; walk.begin(uses, tile_start, n_uses);
    MultUse u; u32 row0;
    bool any_bad = false;
    while (walk.next(&u, &row0)) {                            // uniform over the block
        u32 key[16], wt[16], bad;
        mult_load_tile(u, K, row0, key, wt, &bad);
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
        if (__all(single && (total == 0 || k0 == kl))) {      // one key in the whole wave: one add
            const u64 s = wave_sum(total);
            if ((int)(threadIdx.x & 63) == leader) add(kl, s);
            continue;
        }
        u64 acc = 0; u32 cur = 0;                             // runs of equal keys
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (!wt[i]) continue;
            if (acc && key[i] != cur) { add(cur, acc); acc = 0; }
            cur = key[i]; acc += wt[i];
        }
        if (acc) add(cur, acc);
    }
    if (any_bad) ctl->row_oor = 1;
    if (LDS) {
        __syncthreads();
        for (u32 k = threadIdx.x; k < n_keys; k += MULT_THREADS) {
            u64 s = 0;
            for (u32 c = 0; c < copies; c++) s += lds[c * (n_keys + 1) + k];
            if (s) atomicAdd((unsigned long long*)&counters[k], (unsigned long long)s);
        }
    }
}

__global__ __launch_bounds__(256) void mult_scatter_kernel(ColSet table, PackedKey K, u32 n_rows, u64* __restrict__ counters, u32* __restrict__ d_mult, MultCtl* __restrict__ ctl) {
    const u32 pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n_rows) return;
    u32 key = 0, out = 0;
    for (u32 c = 0; c < K.n_cols; c++) { const u32 x = gld(table.col(c) + pos); key |= x << K.shift[c]; out |= x >> K.bits[c]; }
    if (out) { atomicMin(&ctl->tab_oor_pos, pos); return; }
    const u64 count = atomicExch((unsigned long long*)&counters[key], (unsigned long long)MULT_TAKEN);
    if (count == MULT_TAKEN) { atomicMin(&ctl->tab_dup_key, key); return; }
    gst(d_mult + pos, (u32)(count % P));
}

__global__ __launch_bounds__(256) void mult_residual_kernel(const u64* __restrict__ counters, u32 n_keys, MultCtl* __restrict__ ctl) {
    u64 s = 0;
    for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < n_keys; k += gridDim.x * blockDim.x) { const u64 c = counters[k]; if (c != MULT_TAKEN) s += c; }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long*)&ctl->residual, (unsigned long long)s);
}

// after the scatter pass: a counted row is missing when its key's counter was not taken
__global__ __launch_bounds__(MULT_THREADS) void mult_missing_kernel(const MultUse* __restrict__ uses, const u32* __restrict__ tile_start, u32 n_uses, PackedKey K,
                                                                    const u64* __restrict__ counters, MultCtl* __restrict__ ctl) {
    MultWalk walk; walk.begin(uses, tile_start, n_uses);
    MultUse u; u32 row0;
    u64 n = 0, first = ~(u64)0;
    while (walk.next(&u, &row0)) {
        const u32 use = walk.use;
        u32 key[16], wt[16], bad;
        mult_load_tile(u, K, row0, key, wt, &bad);
#pragma unroll
        for (u32 i = 0; i < 16; i++) {
            const bool miss = ((bad >> i) & 1) || (wt[i] && counters[key[i]] != MULT_TAKEN);
            if (miss) {
                const u64 at = ((u64)use << 32) | (row0 + ((i >> 2) * MULT_THREADS + threadIdx.x) * 4 + (i & 3));
                n++; first = at < first ? at : first;
            }
        }
    }
    if (n) { atomicAdd((unsigned long long*)&ctl->n_missing, (unsigned long long)n); atomicMin((unsigned long long*)&ctl->first_missing, (unsigned long long)first); }
}

}  // namespace nx

using namespace nx;

extern "C" {

int nx_logup_multiplicities(nx_ctx* ctx, const nx_lookup_use* uses, uint32_t n_uses, uint32_t n_key_cols, const uint32_t* key_bits,
                            const uint32_t* const* d_table, uint32_t log_table, uint32_t* d_mult, uint64_t* n_missing,
                            uint32_t* first_missing_use, uint64_t* first_missing_pos) {
    NX_GUARD(ctx);
    const char* who = "nx_logup_multiplicities";
    if (!ctx || !key_bits || !d_table || !d_mult || (n_uses && !uses)) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": NULL argument");
    if (n_key_cols < 1 || n_key_cols > 4) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": 1 to 4 key columns");
    PackedKey K; memset(&K, 0, sizeof K);
    K.n_cols = n_key_cols;
    for (u32 c = 0; c < n_key_cols; c++) {
        if (key_bits[c] < 1 || key_bits[c] > 24) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": key_bits of 1 to 24 per column");
        K.bits[c] = key_bits[c]; K.shift[c] = K.total_bits; K.total_bits += key_bits[c];
    }
    if (K.total_bits > 24) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": the key_bits add up to " + std::to_string(K.total_bits) + ", at most 24");
    if (log_table > K.total_bits)
        return set_err(ctx, NX_ERR_ARG, std::string(who) + ": a table of 2^" + std::to_string(log_table) + " rows has two rows with the same " + std::to_string(K.total_bits) + "-bit key");
    if (n_uses > MULT_MAX_USES) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": at most 65536 uses per call");
    for (u32 c = 0; c < n_key_cols; c++) if (!d_table[c]) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": NULL table column");
    std::vector<MultUse> h_uses(std::max<u32>(1, n_uses));
    std::vector<u32> h_start(n_uses + 1, 0);
    u64 rows = 0;
    for (u32 i = 0; i < n_uses; i++) {
        const nx_lookup_use& s = uses[i];
        if (s.log_size > 30) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": use " + std::to_string(i) + ": log_size too large");
        rows += (u64)1 << s.log_size;
        if (rows > ((u64)1 << 32)) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": more than 2^32 rows in one call");
        if (!s.d_values) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": use " + std::to_string(i) + ": NULL d_values");
        MultUse& u = h_uses[i]; memset(&u, 0, sizeof u);
        const u64 n = (u64)1 << s.log_size;
        uintptr_t align = (uintptr_t)s.d_weight;
        for (u32 c = 0; c < n_key_cols; c++) {
            if (!s.d_values[c]) return set_err(ctx, NX_ERR_ARG, std::string(who) + ": use " + std::to_string(i) + ": NULL value column");
            u.col[c] = s.d_values[c]; align |= (uintptr_t)s.d_values[c];
        }
        u.weight = s.d_weight; u.log_size = s.log_size;
        u.vec = n >= MULT_TILE && !(align & 15);              // whole tiles of aligned columns: 16-byte loads
        h_start[i + 1] = h_start[i] + (u32)((n + MULT_TILE - 1) / MULT_TILE);
    }
    const u32 n_tiles = h_start[n_uses], n_keys = 1u << K.total_bits, n_rows = 1u << log_table;
    // one block: the control words, the use table, the tile starts, the counters
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_ctl = al(sizeof(MultCtl)), b_uses = al(h_uses.size() * sizeof(MultUse)), b_start = al(h_start.size() * 4), b_cnt = (size_t)n_keys * 8;
    uint8_t* blob = nullptr;
    NX_TRY(dev_alloc(ctx, b_ctl + b_uses + b_start + b_cnt, (void**)&blob));
    MultCtl* d_ctl = (MultCtl*)blob; const MultUse* d_uses = (const MultUse*)(blob + b_ctl); const u32* d_start = (const u32*)(blob + b_ctl + b_uses);
    u64* d_cnt = (u64*)(blob + b_ctl + b_uses + b_start);
    MultCtl h_ctl; memset(&h_ctl, 0, sizeof h_ctl);
    h_ctl.first_missing = ~(u64)0; h_ctl.tab_oor_pos = ~0u; h_ctl.tab_dup_key = ~0u;
    ColSet table;
    int rc = make_colset(ctx, d_table, n_key_cols, &table);
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_ctl, &h_ctl, sizeof h_ctl);
    if (rc == NX_OK) rc = upload_async_staged(ctx, (void*)d_uses, h_uses.data(), h_uses.size() * sizeof(MultUse));
    if (rc == NX_OK) rc = upload_async_staged(ctx, (void*)d_start, h_start.data(), h_start.size() * 4);
    if (rc != NX_OK) { dev_free(ctx, blob); return rc; }
    const bool lds = K.total_bits <= NX_MULT_LDS_MAX_KEY_BITS;
    const u32 walk_grid = std::max<u32>(1, std::min<u32>(n_tiles, (u32)ctx->n_cus * 4));
    hipError_t e = hipMemsetAsync(d_cnt, 0, b_cnt, ctx->stream);
    if (e == hipSuccess && n_tiles) {
        if (lds) hipLaunchKernelGGL(mult_count_kernel<true>, dim3(walk_grid), dim3(MULT_THREADS), 0, ctx->stream, d_uses, d_start, n_uses, K, d_cnt, d_ctl);
        else hipLaunchKernelGGL(mult_count_kernel<false>, dim3(walk_grid), dim3(MULT_THREADS), 0, ctx->stream, d_uses, d_start, n_uses, K, d_cnt, d_ctl);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mult_scatter_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, ctx->stream, table, K, n_rows, d_cnt, d_mult, d_ctl);
        hipLaunchKernelGGL(mult_residual_kernel, dim3(std::max<u32>(1, std::min<u32>((n_keys + 255) / 256, (u32)ctx->n_cus * 8))), dim3(256), 0, ctx->stream,
                           (const u64*)d_cnt, n_keys, d_ctl);
        e = hipGetLastError();
    }
    if (e == hipSuccess) rc = copy_d2h_blocking(ctx, &h_ctl, d_ctl, sizeof h_ctl);
    if (e == hipSuccess && rc == NX_OK && h_ctl.tab_oor_pos == ~0u && h_ctl.tab_dup_key == ~0u && (h_ctl.residual || h_ctl.row_oor) && n_tiles) {
        hipLaunchKernelGGL(mult_missing_kernel, dim3(walk_grid), dim3(MULT_THREADS), 0, ctx->stream, d_uses, d_start, n_uses, K, (const u64*)d_cnt, d_ctl);
        e = hipGetLastError();
        if (e == hipSuccess) rc = copy_d2h_blocking(ctx, &h_ctl, d_ctl, sizeof h_ctl);
    }
    dev_free(ctx, blob);                                      // every pass has completed: the copies above block
    if (e != hipSuccess) return hip_fail(ctx, e, who, __FILE__, __LINE__);
    if (rc != NX_OK) return rc;
    if (h_ctl.tab_oor_pos != ~0u)
        return set_err(ctx, NX_ERR_ARG, std::string(who) + ": table row position " + std::to_string(h_ctl.tab_oor_pos) + " holds a value outside its key_bits");
    if (h_ctl.tab_dup_key != ~0u) {
        std::string t;
        for (u32 c = 0; c < n_key_cols; c++) t += (c ? ", " : "") + std::to_string((h_ctl.tab_dup_key >> K.shift[c]) & ((1u << K.bits[c]) - 1));
        return set_err(ctx, NX_ERR_ARG, std::string(who) + ": two table rows hold (" + t + ")");
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
    return set_err(ctx, NX_ERR_PROTOCOL, std::string(who) + ": use " + std::to_string(mu) + " row position " + std::to_string(mp) + ": (" + t + ") is not a row of the table (" +
                                             std::to_string(h_ctl.n_missing) + " such row" + (h_ctl.n_missing == 1 ? "" : "s") + ")");
}

}  // extern "C"
