// The memory-check fillers' shared text: what nx_trace_prev_access (prev_access.hip) and nx_trace_access_chain (access_chain.hip) are made
// of.  ONE text, included inside namespace nx after internal.h, <algorithm>, <string.h>, <string> and <type_traits>; it brings trace_rows.h
// and count_pass.cuh with it.
//
// For every access, what the previous access to the same address left behind.  The reference walks the accesses in time order over a map
// (RegisterMemCheckSideNote::access, prover/src/trace/regs.rs:29-37; ReadWriteMemCheckSideNote::last_access,
// prover/src/trace/sidenote/mod.rs:25-47; program_mem_check.rs:49-96) and reads the final state tables off the map at the end.  Ordered
// by (key, time) it is one data-parallel problem:
//   enumerate  one element per access, written at its TIME INDEX (epoch, natural row, stream, sub-access): the packed key and a 32-bit
//              handle (first element of the stream + storage position); a row that does not access, or refused input (recorded: the
//              smallest ah_bad word), gets the handle AH_NONE, which the last sort pass puts behind every key.  The zeros of the rows that
//              do not access are written here.
//   sort       stable LSD radix sort of the (key, handle) pairs, 8-bit digits: every pass is the counting pass of count_pass.cuh
//              (histogram, scan, stable placement) with the policy AhSort, which takes the digit from the key and moves the pair.
//   resolve    in sorted order element j continues the run of j - 1 or heads a new one: heads are counted and the last head is
//              found per block, both scanned over the blocks (one block), then every element gathers the payload of j - 1 (or
//              init), writes it with its ordinal j - head to its own storage position; heads and tails write the summary entry of
//              their run (index = heads before it; the keys are already ascending).
// Blocks communicate at kernel boundaries only: nothing waits on another block.  Atomics carry integers (LDS histogram adds, one
// 64-bit minimum for refused input).
//
// Every kernel and the host driver are templates on ONE switch.  FULL = false is nx_trace_prev_access: column streams whose accesses know
// in advance what they leave.  FULL = true is nx_trace_access_chain, with two additions that the other instantiation does not carry, as
// kernel argument, allocation or launch:
//   enumerate  a BLOCK stream is a list of records (the keccak instances), record j making `span` accesses to key(j) + i at natural row
//              d_row[j]; the time index of a row of a column stream is the closed formula (ah_time_index) plus, per block stream of its
//              epoch, span x (records before the row): one binary search in d_row, hence at most AH_MAX_BLOCK_STREAMS of them.  A block
//              element adds its own j * span + i.  The host reads the refusal word back BEFORE anything is sorted (a d_row that does not
//              ascend leaves time indices unwritten), so the sort and the resolve see whole permutations only.
//   resolve    a column that is NX_CHAIN_ADD in some stream is a segmented scan over the sorted list with the monoid {set v, add d}:
//              add after add adds, anything after a set is a set, and the head of a run is the set of (init after its own op), so no
//              segment flag is carried: every prefix that ends in or after a head is a set.  Per block of 1024 sorted elements the
//              composition of its ops (is_set, value) is written next to the head count and the last head; one block per chained
//              column scans them over the blocks; the resolve launch composes carry, lanes before and its own quad.  Columns that are
//              NX_CHAIN_GIVEN in every stream gather from element j - 1 and cost nothing extra.

#include "trace_rows.h"
#include "count_pass.cuh"

constexpr u32 AH_THREADS = CP_THREADS, AH_TILE = AH_THREADS * 4;
constexpr u32 AH_NONE = 0xFFFFFFFFu;                             // handle of an element that is no access (handles are < 2^31)
constexpr u32 AH_MAX_STREAMS = 1u << 16, AH_MAX_PAYLOAD = 16, AH_MAX_BLOCK_STREAMS = 8, AH_MAX_SPAN = 256;
constexpr u32 AH_RULE_ADD = NX_CHAIN_ADD, AH_RULE_BYTES = NX_CHAIN_BYTES;
// refused input, as ah_bad records it and ah_bad_read takes it apart (the minimum is the smallest offender)
constexpr u32 AH_BAD_ENTRY = 0, AH_BAD_SUB = 1, AH_BAD_ORDER = 2, AH_BAD_ROW = 3;

struct AhStream {
    const u32* key[4]; const u32* flag; const u32* row; u32* ord;
    u32 log_size, linear, vec, epoch_slot, span, n_records, n_elems;
    uint16_t before_ge[32];     // earlier COLUMN streams of the same epoch with log_size >= L (at most 65535)
};
// column streams of one epoch: ge[b] of them have >= 2^b rows, the others have small[b] rows together; base: first time index of the epoch
struct AhEpoch { u32 base, ge[32], small[32]; };
// the block streams of the call: index in `streams`, epoch slot, records, span, rows
struct AhBlocks { u32 n, stream[AH_MAX_BLOCK_STREAMS], slot[AH_MAX_BLOCK_STREAMS], n_records[AH_MAX_BLOCK_STREAMS], span[AH_MAX_BLOCK_STREAMS]; const u32* row[AH_MAX_BLOCK_STREAMS]; };
struct AhPass { u32 shift, last, sentinel; };                    // digit = (key >> shift) & 255; in the last pass AH_NONE -> sentinel
struct AhInit { u32 w[AH_MAX_PAYLOAD]; };
struct AhSum { u32 cap; u32* key; u32* count; u32* last[AH_MAX_PAYLOAD]; };
struct AhChain { u32 n, mask, col[AH_MAX_PAYLOAD]; };            // the payload columns that are ADD in some stream
struct AhCtl { u64 first_bad; u32 n_keys; u32 pad[13]; };       // one 64-byte block of device memory
struct AhOp { u32 set, val; };                                   // set: the state becomes val; else: val is added to it
// a kernel argument that only the FULL instantiation takes, and how the host passes it.  (A pointer among them is a parameter of its own,
// not a member of one struct of them: only a parameter can promise the compiler that nothing else points to its words.)
struct AhAbsent {};
template <bool FULL, class T> using AhIfFull = std::conditional_t<FULL, T, AhAbsent>;
template <bool FULL, class T> static inline AhIfFull<FULL, T> ah_if_full(T x) { if constexpr (FULL) return x; else return AhAbsent{}; }

__device__ __forceinline__ u32 ah_bitlen(u32 x) { return x ? 32u - (u32)__builtin_clz(x) : 0u; }
__device__ __forceinline__ AhOp ah_then(AhOp a, AhOp b) { AhOp r; r.set = a.set | b.set; r.val = b.set ? b.val : a.val + b.val; return r; }   // a, then b
// FULL: stream << 41 | position or record << 10 | sub-access << 2 | kind.  Without block streams the only kind is AH_BAD_ENTRY of a row and
// the word is stream << 32 | position: the shifted position would cost the enumeration two VGPRs.
template <bool FULL> __device__ __forceinline__ u64 ah_bad(u32 s, u32 at, u32 sub, u32 kind) {
    return FULL ? ((u64)s << 41) | ((u64)at << 10) | ((u64)sub << 2) | kind : ((u64)s << 32) | at;
}
struct AhBad { u32 stream, kind, sub; u64 at; };
template <bool FULL> static inline AhBad ah_bad_read(u64 w) {
    if (FULL) return {(u32)(w >> 41), (u32)(w & 3), (u32)((w >> 2) & 255), (w >> 10) & 0x7FFFFFFFu};
    return {(u32)(w >> 32), AH_BAD_ENTRY, 0, w & 0xFFFFFFFFu};
}

// column-stream elements of the call before (natural row r, stream S of epoch E): those of the epochs before (ebase = E->base, read once
// by the caller); sum over the epoch's column streams of min(r, rows); then the earlier ones that have row r
__device__ __forceinline__ u32 ah_time_index(u32 ebase, const AhEpoch* __restrict__ E, const AhStream& S, u32 r) {
    const u32 b = r ? ah_bitlen(r - 1) : 0;
    return ebase + r * E->ge[b] + E->small[b] + S.before_ge[ah_bitlen(r)];
}
// records of a block stream with d_row < r (inclusive: <= r)
__device__ __forceinline__ u32 ah_records_before(const u32* __restrict__ row, u32 n, u32 r, bool inclusive) {
    u32 lo = 0, hi = n;
    while (lo < hi) { const u32 mid = lo + (hi - lo) / 2; const u32 x = gld(row + mid); if (inclusive ? x <= r : x < r) lo = mid + 1; else hi = mid; }
    return lo;
}
// elements of the OTHER block streams of epoch `slot` that come before (natural row r, stream s)
__device__ __forceinline__ u32 ah_block_elems_before(const AhBlocks& B, u32 slot, u32 s, u32 r) {
    u32 sum = 0;
#pragma unroll
    for (u32 b = 0; b < AH_MAX_BLOCK_STREAMS; b++)
        if (b < B.n && B.slot[b] == slot && B.stream[b] != s) sum += B.span[b] * ah_records_before(B.row[b], B.n_records[b], r, B.stream[b] < s);
    return sum;
}
__device__ __forceinline__ u32 ah_block_elems_before(const AhAbsent&, u32, u32, u32) { return 0u; }
// what access `el` of a stream leaves in a GIVEN column: a word, or byte `el` of the packed records
__device__ __forceinline__ u32 ah_payload(const u32* __restrict__ src, u32 rule, u32 el) {
    if (!src) return 0u;
    if (rule & AH_RULE_BYTES) return (gld(src + (el >> 2)) >> (8 * (el & 3))) & 255u;
    return gld(src + el);
}
// the rule of a (stream, payload column) = at: GIVEN where the call has no rules
__device__ __forceinline__ u32 ah_rule(const u32* __restrict__ rule, size_t at) { return rule[at]; }
__device__ __forceinline__ u32 ah_rule(AhAbsent, size_t) { return NX_CHAIN_GIVEN; }

// One block per tile of 1024 elements of one stream (tile_start: first tile of every stream), four consecutive elements per lane.
template <bool FULL>
__global__ __launch_bounds__(AH_THREADS) void ah_enumerate_kernel(const AhStream* __restrict__ streams, const AhEpoch* __restrict__ epochs, const u32* __restrict__ tile_start,
                                                                  const u32* __restrict__ sbase, u32 n_streams, PackedKey K, AhIfFull<FULL, AhBlocks> B, u32 n_payload,
                                                                  u32* const* __restrict__ prv, u32* __restrict__ keys, u32* __restrict__ vals, AhCtl* __restrict__ ctl) {
    const u32 s = find_le(tile_start, n_streams, blockIdx.x);
    const AhStream& S = streams[s];                 // read where it is: a per-lane copy would put before_ge, indexed at run time, into scratch
    const AhEpoch* __restrict__ E = epochs + S.epoch_slot;
    const u32 n = FULL ? S.n_elems : 1u << S.log_size;   // (column streams alone: the shift, as this kernel had it before it was shared)
    const u32 row0 = (blockIdx.x - tile_start[s]) * AH_TILE + threadIdx.x * 4;
    if (row0 >= n) return;
    const u32 base = gld(sbase + s), ebase = E->base;
    if constexpr (FULL) {
        if (S.row) {
            // a block stream: element el is sub-access i of record j
            const u32 span = S.span;
            for (u32 e = 0; e < 4; e++) {
                const u32 el = row0 + e;
                if (el >= n) break;
                const u32 j = el / span, i = el - j * span;
                const u32 r_raw = gld(S.row + j), r = r_raw & 0x7FFFFFFFu;                   // a row of 2^31 or more is refused below
                const bool access = S.flag ? gld(S.flag + j) != 0 : true;
                u32 k = 0, o = 0;
#pragma unroll
                for (u32 c = 0; c < 4; c++)
                    if (c < K.n_cols) { const u32 x = gld(S.key[c] + j); k |= x << K.shift[c]; o |= K.bits[c] < 32 ? x >> K.bits[c] : 0u; }
                const u64 kk = (u64)k + i;
                const bool bad_entry = access && o != 0, bad_sub = access && !bad_entry && (kk >> K.total_bits) != 0;
                if (i == 0) {
                    if (r_raw >> 31) atomicMin((unsigned long long*)&ctl->first_bad, (unsigned long long)ah_bad<FULL>(s, j, 0, AH_BAD_ROW));
                    else if (j && gld(S.row + j - 1) >= r_raw) atomicMin((unsigned long long*)&ctl->first_bad, (unsigned long long)ah_bad<FULL>(s, j, 0, AH_BAD_ORDER));
                    if (bad_entry) atomicMin((unsigned long long*)&ctl->first_bad, (unsigned long long)ah_bad<FULL>(s, j, 0, AH_BAD_ENTRY));
                }
                if (bad_sub) atomicMin((unsigned long long*)&ctl->first_bad, (unsigned long long)ah_bad<FULL>(s, j, i, AH_BAD_SUB));
                // column-stream elements before (r, s), the other block streams' before (r, s), this stream's own before el
                const u32 idx = ah_time_index(ebase, E, S, r) + ah_block_elems_before(B, S.epoch_slot, s, r) + el;
                const bool ok = access && !bad_entry && !bad_sub;
                gst(keys + idx, ok ? (u32)kk : 0u);
                gst(vals + idx, ok ? base + el : AH_NONE);
                if (!access) {
                    if (S.ord) gst(S.ord + el, 0u);
                    for (u32 c = 0; c < n_payload; c++) { u32* p = prv[(size_t)s * n_payload + c]; if (p) gst(p + el, 0u); }
                }
            }
            return;
        }
    }
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
#pragma unroll
    for (u32 e = 0; e < 4; e++) {
        const u32 pos = row0 + e;
        if (pos >= n) break;
        const u32 r = S.linear ? pos : coset_row_of_pos(pos, (int)S.log_size);
        // column-stream elements before (r, s); the records of the epoch's block streams before (r, s)
        const u32 idx = ah_time_index(ebase, E, S, r) + ah_block_elems_before(B, S.epoch_slot, s, r);
        const bool access = f[e] != 0, bad = access && o[e] != 0, ok = access && !bad;
        if (bad) atomicMin((unsigned long long*)&ctl->first_bad, (unsigned long long)ah_bad<FULL>(s, pos, 0, AH_BAD_ENTRY));
        gst(keys + idx, ok ? k[e] : 0u);
        gst(vals + idx, ok ? base + pos : AH_NONE);
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

__device__ __forceinline__ u32 ah_digit(u32 key, u32 val, AhPass ps) {
    const u32 d = ps.shift < 32 ? (key >> ps.shift) & 255u : 0u;
    return (ps.last && val == AH_NONE) ? ps.sentinel : d;
}

// one pass of the sort as a counting pass: the histogram needs the handle in the last pass only, the placement moves the pair
struct AhSort {
    const u32* kin; const u32* vin; u32* kout; u32* vout; AhPass ps;
    struct Item { u32 key, val; };
    __device__ __forceinline__ bool digit(u32 j, u32 total, u32* d) const {
        const bool have = j < total;
        const u32 key = have ? gld(kin + j) : 0u, val = (have && ps.last) ? gld(vin + j) : 0u;
        *d = have ? ah_digit(key, val, ps) : 0u;
        return have;
    }
    __device__ __forceinline__ bool load(u32 j, u32 total, Item* it, u32* d) const {
        const bool have = j < total;
        it->key = have ? gld(kin + j) : 0u; it->val = have ? gld(vin + j) : 0u;
        *d = have ? ah_digit(it->key, it->val, ps) : 0u;
        return have;
    }
    __device__ __forceinline__ void store(u32 slot, const Item& it) const { gst(kout + slot, it.key); gst(vout + slot, it.val); }
};

// the four sorted elements j0 .. j0 + 3 of a lane with their neighbours: head[e] heads a run, tail[e] ends one, ok[e]: an access
struct AhQuad { u32 key[4], val[4], prev_val; bool head[4], tail[4], ok[4]; };
__device__ __forceinline__ void ah_load_quad(const u32* __restrict__ keys, const u32* __restrict__ vals, u32 total, u32 j0, bool want_tail, AhQuad* q) {
    const bool full = j0 + 3 < total;
    const uint4 kv = gld4_guarded(keys, j0, total, full), vv = gld4_guarded(vals, j0, total, full);
    q->key[0] = kv.x; q->key[1] = kv.y; q->key[2] = kv.z; q->key[3] = kv.w;
    q->val[0] = vv.x; q->val[1] = vv.y; q->val[2] = vv.z; q->val[3] = vv.w;
    u32 pk = 0, pv = AH_NONE;                                 // the element before: an AH_NONE neighbour never continues a run
    if (j0 > 0 && j0 < total) { pk = gld(keys + j0 - 1); pv = gld(vals + j0 - 1); }
    q->prev_val = pv;
    u32 nk = 0, nv = AH_NONE;
    if (want_tail && j0 + 4 < total) { nk = gld(keys + j0 + 4); nv = gld(vals + j0 + 4); }
#pragma unroll
    for (u32 e = 0; e < 4; e++) {
        const bool ok = j0 + e < total && q->val[e] != AH_NONE;
        const u32 bk = e ? q->key[e - 1] : pk, bv = e ? q->val[e - 1] : pv;
        const u32 ak = e < 3 ? q->key[e + 1] : nk, av = (e < 3 ? (j0 + e + 1 < total ? q->val[e + 1] : AH_NONE) : nv);
        q->ok[e] = ok;
        q->head[e] = ok && (bv == AH_NONE || bk != q->key[e]);
        q->tail[e] = ok && (av == AH_NONE || ak != q->key[e]);
    }
}

// exclusive scan of one op per thread over the block's 256 threads in thread order, *total: the whole block's.  lds: 8 words, free again on return.
__device__ __forceinline__ AhOp ah_block_scan(AhOp v, u32* lds, AhOp* total) {
    const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    AhOp inc = v;
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
        AhOp t;
        t.set = __shfl(inc.set, (int)((lane - off) & 63), 64); t.val = __shfl(inc.val, (int)((lane - off) & 63), 64);
        if (lane >= off) inc = ah_then(t, inc);
    }
    if (lane == 63) { lds[2 * w] = inc.set; lds[2 * w + 1] = inc.val; }
    __syncthreads();
    AhOp base = {0, 0}, tot = {0, 0};
#pragma unroll
    for (u32 i = 0; i < 4; i++) { AhOp x; x.set = lds[2 * i]; x.val = lds[2 * i + 1]; if (i < w) base = ah_then(base, x); tot = ah_then(tot, x); }
    __syncthreads();
    AhOp prev;
    prev.set = __shfl(inc.set, (int)((lane - 1) & 63), 64); prev.val = __shfl(inc.val, (int)((lane - 1) & 63), 64);
    *total = tot;
    return lane ? ah_then(base, prev) : base;
}

// the op of sorted element (stream s, access el) in payload column c; the head of a run sets the state to (init, then its op)
__device__ __forceinline__ AhOp ah_op(const u32* const* __restrict__ pay, const u32* __restrict__ rule, const u32* __restrict__ delta, u32 n_payload, u32 s, u32 el, u32 c, bool head,
                                      u32 init) {
    const size_t at = (size_t)s * n_payload + c;
    const u32 ru = rule[at];
    AhOp op;
    if (ru & AH_RULE_ADD) { op.set = head ? 1u : 0u; op.val = (head ? init : 0u) + delta[at]; }
    else { op.set = 1u; op.val = ah_payload(pay[at], ru, el); }
    return op;
}

// per block of 1024 sorted elements: the heads in it and (index + 1) of its last head, 0 = none; FULL: and per chained column the
// composition of its elements' ops
template <bool FULL>
__global__ __launch_bounds__(AH_THREADS) void ah_heads_kernel(const u32* __restrict__ keys, const u32* __restrict__ vals, u32 total, u32* __restrict__ blk_cnt, u32* __restrict__ blk_last,
                                                              const u32* __restrict__ sbase, u32 n_streams, u32 n_payload, const u32* const* __restrict__ pay,
                                                              AhIfFull<FULL, const u32* __restrict__> rule, AhIfFull<FULL, const u32* __restrict__> delta, AhInit init,
                                                              AhIfFull<FULL, AhChain> chain, AhIfFull<FULL, u32* __restrict__> agg_set, AhIfFull<FULL, u32* __restrict__> agg_val) {
    __shared__ u32 lds[FULL ? 8 : 4];
    const u32 j0 = blockIdx.x * AH_TILE + threadIdx.x * 4;
    AhQuad q; ah_load_quad(keys, vals, total, j0, false, &q);
    u32 cnt = 0, last = 0;
#pragma unroll
    for (u32 e = 0; e < 4; e++) if (q.head[e]) { cnt++; last = j0 + e + 1; }
    u32 tc, tl;
    (void)block_scan<0>(cnt, lds, &tc);
    (void)block_scan<1>(last, lds, &tl);
    if (threadIdx.x == 0) { blk_cnt[blockIdx.x] = tc; blk_last[blockIdx.x] = tl; }
    if constexpr (FULL) {
        if (!chain.n) return;
        u32 es[4] = {0, 0, 0, 0}, el[4] = {0, 0, 0, 0};
#pragma unroll
        for (u32 e = 0; e < 4; e++)
            if (q.ok[e]) { es[e] = find_le(sbase, n_streams, q.val[e]); el[e] = q.val[e] - sbase[es[e]]; }
        for (u32 ci = 0; ci < chain.n; ci++) {
            const u32 c = chain.col[ci];
            AhOp st = {0, 0};
#pragma unroll
            for (u32 e = 0; e < 4; e++)
                if (q.ok[e]) st = ah_then(st, ah_op(pay, rule, delta, n_payload, es[e], el[e], c, q.head[e], init.w[c]));
            AhOp tot;
            (void)ah_block_scan(st, lds, &tot);
            if (threadIdx.x == 0) { agg_set[(size_t)ci * gridDim.x + blockIdx.x] = tot.set; agg_val[(size_t)ci * gridDim.x + blockIdx.x] = tot.val; }
        }
    }
}

// in-place exclusive scan of the blocks' ops, one block per chained column (a template like the others, so that only the file that
// launches it holds it)
template <bool FULL>
__global__ __launch_bounds__(AH_THREADS) void ah_scan_ops_kernel(u32* __restrict__ agg_set, u32* __restrict__ agg_val, u32 n) {
    __shared__ u32 lds[8];
    u32* set = agg_set + (size_t)blockIdx.x * n; u32* val = agg_val + (size_t)blockIdx.x * n;
    AhOp carry = {0, 0};
    for (u32 base = 0; base < n; base += AH_THREADS) {
        const u32 i = base + threadIdx.x;
        AhOp v = {0, 0};
        if (i < n) { v.set = set[i]; v.val = val[i]; }
        AhOp tot;
        const AhOp ex = ah_then(carry, ah_block_scan(v, lds, &tot));
        if (i < n) { set[i] = ex.set; val[i] = ex.val; }
        carry = ah_then(carry, tot);
    }
}

// blk_cnt / blk_last: scanned over the blocks (heads before the block; last head before the block); FULL: the aggregates are scanned too
// (the state op of everything before the block).  sbase: first handle of every stream; pay / prv / rule / delta: [stream][payload column].
template <bool FULL>
__global__ __launch_bounds__(AH_THREADS) void ah_resolve_kernel(const u32* __restrict__ keys, const u32* __restrict__ vals, u32 total, const u32* __restrict__ blk_cnt,
                                                                const u32* __restrict__ blk_last, const AhStream* __restrict__ streams, const u32* __restrict__ sbase, u32 n_streams,
                                                                u32 n_payload, const u32* const* __restrict__ pay, u32* const* __restrict__ prv,
                                                                AhIfFull<FULL, const u32* __restrict__> rule, AhIfFull<FULL, const u32* __restrict__> delta, AhInit init, AhSum sum,
                                                                AhIfFull<FULL, AhChain> chain, AhIfFull<FULL, const u32* __restrict__> agg_set,
                                                                AhIfFull<FULL, const u32* __restrict__> agg_val) {
    __shared__ u32 lds[FULL ? 8 : 4];
    const u32 j0 = blockIdx.x * AH_TILE + threadIdx.x * 4;
    AhQuad q; ah_load_quad(keys, vals, total, j0, true, &q);
    u32 cnt = 0, last = 0;
#pragma unroll
    for (u32 e = 0; e < 4; e++) if (q.head[e]) { cnt++; last = j0 + e + 1; }
    u32 unused;
    u32 seg = blk_cnt[blockIdx.x] + block_scan<0>(cnt, lds, &unused);              // heads before this lane's elements
    u32 start = scan_op<1>(blk_last[blockIdx.x], block_scan<1>(last, lds, &unused)); // (index + 1) of the last head before them
    u32 es[4] = {0, 0, 0, 0}, el[4] = {0, 0, 0, 0}, erun[4] = {0, 0, 0, 0};
    bool to_sum[4] = {false, false, false, false};
    u32 mask = 0;                                                // the chained columns: none without rules
    if constexpr (FULL) mask = chain.mask;
#pragma unroll
    for (u32 e = 0; e < 4; e++) {
        const u32 j = j0 + e;
        // The rows that do not access are sorted last, so as a rule nothing follows the first AH_NONE.  One exception, on the path that sorts
        // refused rows (FULL = false): a call without any d_flag and with whole-byte keys has AH_NONE only on REFUSED rows, which share digit
        // 255 with real keys and may lie between them; the call then returns NX_ERR_PROTOCOL and its outputs are unspecified.  Such an element
        // is skipped and those behind it are resolved: that stays in bounds, because ah_load_quad lets no run continue across an AH_NONE
        // (the element behind one is a head), so find_le sees handles of accesses only and an ordinal counts from a head of real elements.
        if (!q.ok[e]) continue;
        if (q.head[e]) { seg++; start = j + 1; }
        const u32 run = seg - 1, ordinal = j + 1 - start;
        const u32 s = find_le(sbase, n_streams, q.val[e]), pos = q.val[e] - sbase[s];
        es[e] = s; el[e] = pos; erun[e] = run;
        const u32 pval = e ? q.val[e - 1] : q.prev_val;
        u32 ps = 0, ppos = 0;
        if (!q.head[e]) { ps = find_le(sbase, n_streams, pval); ppos = pval - sbase[ps]; }
        u32* ord = streams[s].ord;
        if (ord) gst(ord + pos, ordinal);
        to_sum[e] = q.tail[e] && run < sum.cap;
        if (q.head[e] && run < sum.cap && sum.key) gst(sum.key + run, q.key[e]);
        if (to_sum[e] && sum.count) gst(sum.count + run, ordinal + 1);
        for (u32 c = 0; c < n_payload; c++) {
            if ((mask >> c) & 1) continue;
            u32* dst = prv[(size_t)s * n_payload + c];
            if (dst) {
                u32 x = init.w[c];
                if (!q.head[e]) x = ah_payload(pay[(size_t)ps * n_payload + c], ah_rule(rule, (size_t)ps * n_payload + c), ppos);
                gst(dst + pos, x);
            }
            if (to_sum[e] && sum.last[c]) gst(sum.last[c] + run, ah_payload(pay[(size_t)s * n_payload + c], ah_rule(rule, (size_t)s * n_payload + c), pos));
        }
    }
    if constexpr (FULL) {
        for (u32 ci = 0; ci < chain.n; ci++) {
            const u32 c = chain.col[ci];
            AhOp op[4], mine = {0, 0};
#pragma unroll
            for (u32 e = 0; e < 4; e++) {
                op[e].set = 0; op[e].val = 0;
                if (q.ok[e]) op[e] = ah_op(pay, rule, delta, n_payload, es[e], el[e], c, q.head[e], init.w[c]);
                mine = ah_then(mine, op[e]);
            }
            AhOp carry, tot;
            carry.set = agg_set[(size_t)ci * gridDim.x + blockIdx.x]; carry.val = agg_val[(size_t)ci * gridDim.x + blockIdx.x];
            AhOp st = ah_then(carry, ah_block_scan(mine, lds, &tot));                   // everything before this lane's elements
#pragma unroll
            for (u32 e = 0; e < 4; e++) {
                if (!q.ok[e]) continue;
                u32* dst = prv[(size_t)es[e] * n_payload + c];
                if (dst) gst(dst + el[e], q.head[e] ? init.w[c] : st.val);
                st = ah_then(st, op[e]);
                if (to_sum[e] && sum.last[c]) gst(sum.last[c] + erun[e], st.val);
            }
        }
    }
}

// Both entries.  `streams` has the shape of nx_trace_access_chain's; FULL = false takes column streams without rules (d_row, rule and
// delta NULL) and says "rows" where the other says "elements".
template <bool FULL>
static int access_history(nx_ctx* ctx, const std::string& who, const nx_chain_stream* streams, u32 n_streams, u32 n_key_cols, const u32* key_bits, u32 n_payload, const u32* init,
                          const nx_access_summary* summary, u64* n_keys) {
    // every refusal is decided from host memory alone; the NULL context comes last so that each of them can be met without a device
    if (!streams) return set_err(ctx, NX_ERR_ARG, who + ": NULL streams");
    if (!key_bits) return set_err(ctx, NX_ERR_ARG, who + ": NULL key_bits");
    if (n_streams < 1 || n_streams > AH_MAX_STREAMS) return set_err(ctx, NX_ERR_ARG, who + ": n_streams of " + std::to_string(n_streams) + ", 1 to 65536");
    if (n_key_cols < 1 || n_key_cols > 4) return set_err(ctx, NX_ERR_ARG, who + ": n_key_cols of " + std::to_string(n_key_cols) + ", 1 to 4");
    if (n_payload < 1 || n_payload > AH_MAX_PAYLOAD) return set_err(ctx, NX_ERR_ARG, who + ": n_payload of " + std::to_string(n_payload) + ", 1 to 16");
    PackedKey K; memset(&K, 0, sizeof K);
    K.n_cols = n_key_cols;
    for (u32 c = 0; c < n_key_cols; c++) {
        if (key_bits[c] < 1 || key_bits[c] > 32) return set_err(ctx, NX_ERR_ARG, who + ": key_bits[" + std::to_string(c) + "] of " + std::to_string(key_bits[c]) + ", 1 to 32");
        K.bits[c] = key_bits[c]; K.shift[c] = K.total_bits; K.total_bits += key_bits[c];
        if (K.total_bits > 32) return set_err(ctx, NX_ERR_ARG, who + ": the key_bits add up to more than 32");
    }
    AhInit h_init; memset(&h_init, 0, sizeof h_init);
    for (u32 c = 0; init && c < n_payload; c++) {
        if (init[c] >= P) return set_err(ctx, NX_ERR_ARG, who + ": init[" + std::to_string(c) + "] is not below p");
        h_init.w[c] = init[c];
    }
    // streams: sizes, rules, pointers, aliasing
    std::vector<const void*> ins, outs;
    u64 elems = 0;
    u32 n_block = 0;
    bool any_flag = false;
    AhChain h_chain; memset(&h_chain, 0, sizeof h_chain);
    for (u32 i = 0; i < n_streams; i++) {
        const nx_chain_stream& s = streams[i];
        const std::string at = who + ": stream " + std::to_string(i);
        const bool block = s.d_row != nullptr;
        if (block) {
            if (s.span < 1 || s.span > AH_MAX_SPAN) return set_err(ctx, NX_ERR_ARG, at + ": span of " + std::to_string(s.span) + ", 1 to 256");
            if (++n_block > AH_MAX_BLOCK_STREAMS) return set_err(ctx, NX_ERR_ARG, at + ": more than 8 block streams (streams with a d_row)");
            elems += (u64)s.n_records * s.span;
            ins.push_back(s.d_row);
        } else {
            if (s.log_size > 30 || (!s.linear && s.log_size < 1))
                return set_err(ctx, NX_ERR_ARG, at + ": log_size of " + std::to_string(s.log_size) + (s.linear ? ", 0 to 30 for a linear stream" : ", 1 to 30"));
            elems += (u64)1 << s.log_size;
        }
        if (elems >= ((u64)1 << 31))
            return set_err(ctx, NX_ERR_ARG, who + (FULL ? ": 2^31 elements or more in all (rows, or n_records * span, of stream " : ": 2^31 rows or more in all (log_size of stream ") +
                                                std::to_string(i) + ")");
        for (u32 c = 0; c < n_payload; c++) {
            const u32 ru = s.rule ? s.rule[c] : NX_CHAIN_GIVEN;
            const std::string rc_at = at + ": rule[" + std::to_string(c) + "]";
            if (ru > (NX_CHAIN_ADD | NX_CHAIN_BYTES)) return set_err(ctx, NX_ERR_ARG, rc_at + " of " + std::to_string(ru) + " is no rule");
            if (ru & NX_CHAIN_BYTES) {
                if (ru & NX_CHAIN_ADD) return set_err(ctx, NX_ERR_ARG, rc_at + ": NX_CHAIN_BYTES on an NX_CHAIN_ADD column");
                if (!block) return set_err(ctx, NX_ERR_ARG, rc_at + ": NX_CHAIN_BYTES on a column stream");
                if (s.span % 4) return set_err(ctx, NX_ERR_ARG, rc_at + ": NX_CHAIN_BYTES with a span of " + std::to_string(s.span) + ", no multiple of 4");
                if (s.d_payload && ((uintptr_t)s.d_payload[c] & 3)) return set_err(ctx, NX_ERR_ARG, rc_at + ": NX_CHAIN_BYTES with a d_payload that is not 4-byte aligned");
            }
            if ((ru & NX_CHAIN_ADD) && s.d_payload && s.d_payload[c]) return set_err(ctx, NX_ERR_ARG, rc_at + ": NX_CHAIN_ADD with a d_payload[" + std::to_string(c) + "] that is not NULL");
            if ((ru & NX_CHAIN_ADD) && !((h_chain.mask >> c) & 1)) { h_chain.mask |= 1u << c; }
        }
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
    for (u32 c = 0; c < n_payload; c++) if ((h_chain.mask >> c) & 1) h_chain.col[h_chain.n++] = c;
    AhSum h_sum; memset(&h_sum, 0, sizeof h_sum);
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
    const u32 total = (u32)elems;
    if (!total) { if (n_keys) *n_keys = 0; return NX_OK; }   // block streams without records only: no element, no output word

    // epochs in ascending order; the streams of an epoch keep their array order
    std::vector<u32> ep(n_streams);
    for (u32 i = 0; i < n_streams; i++) ep[i] = streams[i].epoch;
    std::sort(ep.begin(), ep.end()); ep.erase(std::unique(ep.begin(), ep.end()), ep.end());
    std::vector<AhEpoch> h_ep(ep.size());
    std::vector<std::vector<u32>> cnt_log(ep.size(), std::vector<u32>(32, 0));
    std::vector<u32> blk_elems(ep.size(), 0);
    std::vector<AhStream> h_st(n_streams);
    std::vector<u32> h_tile(n_streams + 1, 0), h_base(n_streams + 1, 0);
    std::vector<const u32*> h_pay((size_t)n_streams * n_payload, nullptr);
    std::vector<u32*> h_prv((size_t)n_streams * n_payload, nullptr);
    std::vector<u32> h_rule(FULL ? (size_t)n_streams * n_payload : 0, 0), h_delta(h_rule.size(), 1);
    AhBlocks h_blk; memset(&h_blk, 0, sizeof h_blk);
    for (u32 i = 0; i < n_streams; i++) {
        const nx_chain_stream& s = streams[i];
        AhStream& d = h_st[i]; memset(&d, 0, sizeof d);
        const u32 slot = (u32)(std::lower_bound(ep.begin(), ep.end(), s.epoch) - ep.begin());
        const bool block = s.d_row != nullptr;
        const u64 n = block ? (u64)s.n_records * s.span : (u64)1 << s.log_size;
        uintptr_t align = (uintptr_t)s.d_flag | (uintptr_t)s.d_ordinal;
        for (u32 c = 0; c < n_key_cols; c++) { d.key[c] = s.d_key[c]; align |= (uintptr_t)s.d_key[c]; }
        for (u32 c = 0; c < n_payload; c++) {
            const size_t at = (size_t)i * n_payload + c;
            h_pay[at] = s.d_payload ? s.d_payload[c] : nullptr;
            h_prv[at] = s.d_prev ? s.d_prev[c] : nullptr;
            if (FULL) { h_rule[at] = s.rule ? s.rule[c] : NX_CHAIN_GIVEN; h_delta[at] = s.delta ? s.delta[c] : 1u; }
            align |= (uintptr_t)h_prv[at];
        }
        d.flag = s.d_flag; d.ord = s.d_ordinal; d.row = s.d_row; d.epoch_slot = slot; d.n_elems = (u32)n;
        if (block) { d.span = s.span; d.n_records = s.n_records; }
        else { d.log_size = s.log_size; d.linear = s.linear != 0; d.vec = n >= 4 && !(align & 15); }   // aligned columns of whole quads: 16-byte loads and stores
        u32 ge = 0;                                               // earlier column streams of the epoch with log_size >= L
        for (int L = 31; L >= 0; L--) { ge += cnt_log[slot][L]; d.before_ge[L] = (uint16_t)ge; }
        if (block) {
            const u32 b = h_blk.n++;
            h_blk.stream[b] = i; h_blk.slot[b] = slot; h_blk.n_records[b] = s.n_records; h_blk.span[b] = s.span; h_blk.row[b] = s.d_row;
            blk_elems[slot] += (u32)n;
        } else cnt_log[slot][s.log_size]++;
        h_tile[i + 1] = h_tile[i] + (u32)((n + AH_TILE - 1) / AH_TILE);
        h_base[i + 1] = h_base[i] + (u32)n;
    }
    u32 ebase = 0;
    for (size_t g = 0; g < ep.size(); g++) {
        AhEpoch& e = h_ep[g]; memset(&e, 0, sizeof e);
        e.base = ebase;
        for (u32 b = 0; b < 32; b++)
            for (u32 L = 0; L < 32; L++) { if (L >= b) e.ge[b] += cnt_log[g][L]; else e.small[b] += cnt_log[g][L] << L; }
        ebase += e.small[31] + (cnt_log[g][31] << 31) + blk_elems[g];   // every stream has fewer than 2^31 rows
    }
    const CountPlan plan = count_plan(elems);
    const u32 res_blocks = (total + AH_TILE - 1) / AH_TILE;
    const u32 n_pass = any_flag ? K.total_bits / 8 + 1 : (K.total_bits + 7) / 8;

    // one scratch block; the rules and the aggregates are the FULL path's alone
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_ctl = al(sizeof(AhCtl)), b_st = al(h_st.size() * sizeof(AhStream)), b_ep = al(h_ep.size() * sizeof(AhEpoch)), b_tile = al(h_tile.size() * 4),
                 b_base = al(h_base.size() * 4), b_ptr = al(h_pay.size() * sizeof(void*)), b_rule = al(h_rule.size() * 4), b_elems = al((size_t)total * 4),
                 b_hist = al((size_t)plan.blocks * 256 * 4), b_blk = al((size_t)res_blocks * 4),
                 b_agg = FULL ? al((size_t)res_blocks * 4 * std::max<u32>(1, h_chain.n)) : 0;
    uint8_t* blob = nullptr;
    NX_TRY(dev_alloc(ctx, b_ctl + b_st + b_ep + b_tile + b_base + 2 * b_ptr + 2 * b_rule + 4 * b_elems + b_hist + 2 * b_blk + 2 * b_agg, (void**)&blob));
    uint8_t* at = blob;
    auto take = [&](size_t bytes) { uint8_t* p = at; at += bytes; return p; };
    AhCtl* d_ctl = (AhCtl*)take(b_ctl);
    AhStream* d_st = (AhStream*)take(b_st); AhEpoch* d_ep = (AhEpoch*)take(b_ep);
    u32* d_tile = (u32*)take(b_tile); u32* d_base = (u32*)take(b_base);
    const u32** d_pay = (const u32**)take(b_ptr); u32** d_prv = (u32**)take(b_ptr);
    u32* d_rule = (u32*)take(b_rule); u32* d_delta = (u32*)take(b_rule);
    u32* d_k[2]; u32* d_v[2];
    d_k[0] = (u32*)take(b_elems); d_v[0] = (u32*)take(b_elems); d_k[1] = (u32*)take(b_elems); d_v[1] = (u32*)take(b_elems);
    u32* d_hist = (u32*)take(b_hist); u32* d_cnt = (u32*)take(b_blk); u32* d_last = (u32*)take(b_blk);
    u32* d_aset = (u32*)take(b_agg); u32* d_aval = (u32*)take(b_agg);
    AhCtl h_ctl; memset(&h_ctl, 0, sizeof h_ctl); h_ctl.first_bad = ~(u64)0;
    int rc = upload_async_staged(ctx, d_ctl, &h_ctl, sizeof h_ctl);
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_st, h_st.data(), h_st.size() * sizeof(AhStream));
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_ep, h_ep.data(), h_ep.size() * sizeof(AhEpoch));
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_tile, h_tile.data(), h_tile.size() * 4);
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_base, h_base.data(), h_base.size() * 4);
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_pay, h_pay.data(), h_pay.size() * sizeof(void*));
    if (rc == NX_OK) rc = upload_async_staged(ctx, d_prv, h_prv.data(), h_prv.size() * sizeof(void*));
    if (FULL && rc == NX_OK) rc = upload_async_staged(ctx, d_rule, h_rule.data(), h_rule.size() * 4);
    if (FULL && rc == NX_OK) rc = upload_async_staged(ctx, d_delta, h_delta.data(), h_delta.size() * 4);
    if (rc != NX_OK) { dev_free(ctx, blob); return rc; }

    hipLaunchKernelGGL(ah_enumerate_kernel<FULL>, dim3(h_tile[n_streams]), dim3(AH_THREADS), 0, ctx->stream, (const AhStream*)d_st, (const AhEpoch*)d_ep, (const u32*)d_tile,
                       (const u32*)d_base, n_streams, K, ah_if_full<FULL>(h_blk), n_payload, (u32* const*)d_prv, d_k[0], d_v[0], d_ctl);
    hipError_t e = hipGetLastError();
    // FULL reads refused input back before the sort: a d_row that does not ascend leaves time indices unwritten, and nothing may follow the
    // handles of such a buffer.  The copy blocks, so the enumeration has completed.  Without block streams every time index is written, a
    // refused row is an AH_NONE like a row that does not access, and the call keeps to the one blocking copy at its end.
    bool stop = false;
    if (FULL && e == hipSuccess) { rc = copy_d2h_blocking(ctx, &h_ctl, d_ctl, sizeof h_ctl); stop = rc != NX_OK || h_ctl.first_bad != ~(u64)0; }
    u32 cur = 0;
    for (u32 p = 0; p < n_pass && e == hipSuccess && !stop; p++) {
        AhPass ps; ps.shift = 8 * p; ps.last = p + 1 == n_pass; ps.sentinel = std::min<u32>(255u, 1u << (K.total_bits - 8 * (n_pass - 1)));
        // (255 only without any d_flag and with whole-byte keys: AH_NONE is then a refused row alone, whose place does not matter)
        const AhSort sort = {d_k[cur], d_v[cur], d_k[cur ^ 1], d_v[cur ^ 1], ps};
        e = count_pass(ctx, sort, total, plan, 256, d_hist, nullptr, nullptr);
        cur ^= 1;
    }
    if (e == hipSuccess && !stop) {
        hipLaunchKernelGGL(ah_heads_kernel<FULL>, dim3(res_blocks), dim3(AH_THREADS), 0, ctx->stream, (const u32*)d_k[cur], (const u32*)d_v[cur], total, d_cnt, d_last,
                           (const u32*)d_base, n_streams, n_payload, (const u32* const*)d_pay, ah_if_full<FULL>((const u32*)d_rule), ah_if_full<FULL>((const u32*)d_delta), h_init,
                           ah_if_full<FULL>(h_chain), ah_if_full<FULL>(d_aset), ah_if_full<FULL>(d_aval));
        hipLaunchKernelGGL(scan_kernel<0>, dim3(1), dim3(AH_THREADS), 0, ctx->stream, d_cnt, res_blocks, &d_ctl->n_keys);
        hipLaunchKernelGGL(scan_kernel<1>, dim3(1), dim3(AH_THREADS), 0, ctx->stream, d_last, res_blocks, (u32*)nullptr);
        if constexpr (FULL) if (h_chain.n) hipLaunchKernelGGL(ah_scan_ops_kernel<FULL>, dim3(h_chain.n), dim3(AH_THREADS), 0, ctx->stream, d_aset, d_aval, res_blocks);
        hipLaunchKernelGGL(ah_resolve_kernel<FULL>, dim3(res_blocks), dim3(AH_THREADS), 0, ctx->stream, (const u32*)d_k[cur], (const u32*)d_v[cur], total, (const u32*)d_cnt,
                           (const u32*)d_last, (const AhStream*)d_st, (const u32*)d_base, n_streams, n_payload, (const u32* const*)d_pay, (u32* const*)d_prv, ah_if_full<FULL>((const u32*)d_rule),
                           ah_if_full<FULL>((const u32*)d_delta), h_init, h_sum, ah_if_full<FULL>(h_chain), ah_if_full<FULL>((const u32*)d_aset), ah_if_full<FULL>((const u32*)d_aval));
        e = hipGetLastError();
        if (e == hipSuccess) rc = copy_d2h_blocking(ctx, &h_ctl, d_ctl, sizeof h_ctl);
    }
    // The copies above block, so every launch has completed.  Where a launch failed the copy is skipped and earlier kernels may still
    // run: the block then goes back to the context's cache, whose reuse is ordered on ctx->stream behind them.
    dev_free(ctx, blob);
    if (e != hipSuccess) return hip_fail(ctx, e, who.c_str(), __FILE__, __LINE__);
    if (rc != NX_OK) return rc;
    if (h_ctl.first_bad != ~(u64)0) {
        const AhBad bad = ah_bad_read<FULL>(h_ctl.first_bad);
        const u32 bs = bad.stream, kind = bad.kind, sub = bad.sub;
        const u64 bp = bad.at;
        const bool block = streams[bs].d_row != nullptr;
        const std::string where = who + ": stream " + std::to_string(bs) + (block ? " record " : " row position ") + std::to_string(bp);
        if (kind == AH_BAD_ROW || kind == AH_BAD_ORDER) {
            u32 r[2] = {0, 0};
            NX_TRY(copy_d2h_blocking(ctx, &r[1], streams[bs].d_row + bp, 4));
            if (kind == AH_BAD_ROW) return set_err(ctx, NX_ERR_PROTOCOL, where + ": d_row of " + std::to_string(r[1]) + " is not below 2^31");
            NX_TRY(copy_d2h_blocking(ctx, &r[0], streams[bs].d_row + bp - 1, 4));
            return set_err(ctx, NX_ERR_PROTOCOL, where + ": d_row of " + std::to_string(r[1]) + " is not above its predecessor's " + std::to_string(r[0]) + " (strictly ascending rows)");
        }
        u64 key = 0;
        for (u32 c = 0; c < n_key_cols; c++) {                    // the row's or record's k words, nothing else
            u32 x = 0;
            NX_TRY(copy_d2h_blocking(ctx, &x, streams[bs].d_key[c] + bp, 4));
            if (kind == AH_BAD_ENTRY && K.bits[c] < 32 && (x >> K.bits[c]))
                return set_err(ctx, NX_ERR_PROTOCOL, where + ": key entry " + std::to_string(c) + " holds " + std::to_string(x) + ", outside its " + std::to_string(K.bits[c]) + " bits");
            key |= (u64)x << K.shift[c];
        }
        if (kind == AH_BAD_SUB)
            return set_err(ctx, NX_ERR_PROTOCOL, where + " sub-access " + std::to_string(sub) + ": key " + std::to_string(key) + " + " + std::to_string(sub) + " is outside the " +
                                                     std::to_string(K.total_bits) + " key bits");
        return set_err(ctx, NX_ERR_PROTOCOL, where + ": a key entry outside its bits");
    }
    if (n_keys) *n_keys = h_ctl.n_keys;
    return NX_OK;
}
