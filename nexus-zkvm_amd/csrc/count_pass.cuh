// One stable 8-bit counting pass over `total` elements, shared by the trace fillers that sort or partition on the device (access_history.cuh:
// every pass of its LSD radix sort; trace_partition.hip: its one pass over the class column).  ONE text, included inside namespace nx
// after internal.h and <algorithm>.  Three launches, blocks communicate at the kernel boundaries only:
//   histogram   a block takes tiles * 256 consecutive elements and counts its digits: hist[digit * blocks + block].
//   scan        exclusive sum of the [digit][block] counts by one block, in place: the first output slot of every (digit, block).
//   placement   the same walk again; every element goes to run[digit] + its rank among the block's elements of that digit so far.
// Inside a block a wave ranks its 64 elements with 8 ballots (the mask of the lanes that hold my digit; rank = its popcount below my
// lane), so equal digits — whole-zero byte limbs, the long runs of one opcode — are combined before they meet an LDS counter: one lane
// per distinct digit and wave touches LDS, and the placement uses plain LDS stores, no atomic at all.  Elements leave in the order they
// came in: by tile, by wave, by lane.
//
// What differs between the users is a POLICY object passed by value to both kernels:
//   bool digit(u32 j, u32 total, u32* d) const           histogram: is j an element, and its digit (below the launch's `rows`)
//   Item; bool load(u32 j, u32 total, Item* it, u32* d) const   placement: the same, with what is to be moved
//   void store(u32 slot, const Item& it) const           placement: the element at its slot
// The two walks must agree on elements and digits.  Its pointers are generic inside the struct: read and write through gld / gst.

constexpr u32 CP_THREADS = 256, CP_MIN_TILES = 4;
// a block takes CP_MIN_TILES tiles of 256 elements while that needs at most CP_MAX_BLOCKS blocks, more tiles beyond (2^20 elements by
// the defaults; the host emulations build a second time with a cap of 2 to reach that path at a small size)
#ifndef NX_COUNT_PASS_MAX_BLOCKS
#define NX_COUNT_PASS_MAX_BLOCKS 1024
#endif
constexpr u32 CP_MAX_BLOCKS = NX_COUNT_PASS_MAX_BLOCKS;

struct CountPlan { u32 tiles, blocks; };        // the histogram scratch of a pass is rows * blocks words
static inline CountPlan count_plan(u64 total) {
    CountPlan p;
    p.tiles = std::max<u32>(CP_MIN_TILES, (u32)((total + (u64)CP_THREADS * CP_MAX_BLOCKS - 1) / ((u64)CP_THREADS * CP_MAX_BLOCKS)));
    p.blocks = (u32)((total + (u64)p.tiles * CP_THREADS - 1) / ((u64)p.tiles * CP_THREADS));
    return p;
}

// last index i < n with a[i] <= x (a ascending, a[0] <= x)
__device__ __forceinline__ u32 find_le(const u32* __restrict__ a, u32 n, u32 x) {
    u32 lo = 0, hi = n;
    while (hi - lo > 1) { const u32 mid = (lo + hi) / 2; if (a[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

// the lanes of this wave that hold digit d (lanes without an element hold none and are in no mask)
__device__ __forceinline__ u64 wave_match(u32 d, bool have) {
    u64 m = __ballot(have);
#pragma unroll
    for (u32 b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1;
        const u64 bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

template <int OP> __device__ __forceinline__ u32 scan_op(u32 a, u32 b) { return OP ? (a > b ? a : b) : a + b; }   // 0: sum, 1: maximum; 0 is neutral for both

// exclusive scan of one value per thread over the block's 256 threads, *total: over the whole block.  lds: 4 words, free again on return.
template <int OP> __device__ __forceinline__ u32 block_scan(u32 v, u32* lds, u32* total) {
    const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u32 inc = v;
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
        const u32 t = __shfl(inc, (int)((lane - off) & 63), 64);
        if (lane >= off) inc = scan_op<OP>(inc, t);
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (u32 i = 0; i < 4; i++) { const u32 x = lds[i]; if (i < w) base = scan_op<OP>(base, x); tot = scan_op<OP>(tot, x); }
    __syncthreads();
    const u32 prev = __shfl(inc, (int)((lane - 1) & 63), 64);
    *total = tot;
    return lane ? scan_op<OP>(base, prev) : base;
}

// in-place exclusive scan of a[0 .. n) by ONE block, 16 bytes per lane: a must be 16-byte aligned (every array handed to it is the
// 256-byte aligned part of a scratch block); *total_out (optional): the scan over everything
template <int OP> __global__ __launch_bounds__(CP_THREADS) void scan_kernel(u32* __restrict__ a, u32 n, u32* __restrict__ total_out) {
    __shared__ u32 lds[4];
    u32 carry = 0;
    for (u32 base = 0; base < n; base += CP_THREADS * 4) {
        const u32 i = base + threadIdx.x * 4;
        const uint4 v = gld4_guarded(a, i, n, i + 3 < n);
        const u32 x0 = v.x, x1 = scan_op<OP>(x0, v.y), x2 = scan_op<OP>(x1, v.z), x3 = scan_op<OP>(x2, v.w);
        u32 tot;
        const u32 run = scan_op<OP>(carry, block_scan<OP>(x3, lds, &tot));
        const uint4 out = make_uint4(run, scan_op<OP>(run, x0), scan_op<OP>(run, x1), scan_op<OP>(run, x2));
        if (i + 3 < n) gst4(a + i, out);
        else {
            if (i < n) gst(a + i, out.x);
            if (i + 1 < n) gst(a + i + 1, out.y);
            if (i + 2 < n) gst(a + i + 2, out.z);
        }
        carry = scan_op<OP>(carry, tot);
    }
    if (threadIdx.x == 0 && total_out) *total_out = carry;
}

// hist[digit * blocks + block] for the digits below rows (<= 256): elements of the block's tiles with that digit
template <class POL> __global__ __launch_bounds__(CP_THREADS) void count_hist_kernel(POL pol, u32 total, u32 tiles, u32 rows, u32* __restrict__ hist) {
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63;
    for (u32 t = 0; t < tiles; t++) {
        const u32 j = (blockIdx.x * tiles + t) * CP_THREADS + threadIdx.x;
        u32 d;
        const bool have = pol.digit(j, total, &d);
        const u64 m = wave_match(d, have);
        if (have && !(m & (((u64)1 << lane) - 1))) atomicAdd(&h[d], (u32)__popcll(m));     // the lowest lane of every digit of the wave
    }
    __syncthreads();
    if (threadIdx.x < rows) hist[threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// offs: the scanned histogram.  start_out (optional): rows words, the first slot of every digit, written by block 0.
template <class POL> __global__ __launch_bounds__(CP_THREADS) void count_place_kernel(POL pol, u32 total, u32 tiles, u32 rows, const u32* __restrict__ offs, u32* __restrict__ start_out) {
    __shared__ u32 run[256];            // next free output slot of every digit
    __shared__ u32 wc[2][4][256];       // per tile parity and wave: elements with the digit (zero outside the tile that fills it)
    const u32 first = threadIdx.x < rows ? offs[threadIdx.x * gridDim.x + blockIdx.x] : 0u;
    run[threadIdx.x] = first;
    if (start_out && blockIdx.x == 0 && threadIdx.x < rows) start_out[threadIdx.x] = first;
    for (u32 i = 0; i < 8; i++) (&wc[0][0][0])[i * 256 + threadIdx.x] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (u32 t = 0; t < tiles; t++) {
        const u32 par = t & 1;
        const u32 j = (blockIdx.x * tiles + t) * CP_THREADS + threadIdx.x;
        typename POL::Item it;
        u32 d;
        const bool have = pol.load(j, total, &it, &d);
        const u64 m = wave_match(d, have);
        const u32 rank = (u32)__popcll(m & (((u64)1 << lane) - 1));
        if (have && rank == 0) wc[par][w][d] = (u32)__popcll(m);
        __syncthreads();
        if (have) {
            u32 o = run[d] + rank;
            for (u32 i = 0; i < w; i++) o += wc[par][i][d];
            pol.store(o, it);
        }
        __syncthreads();
        const u32 s = wc[par][0][threadIdx.x] + wc[par][1][threadIdx.x] + wc[par][2][threadIdx.x] + wc[par][3][threadIdx.x];
        if (s) {   // thread t owns digit t; these words are next written two tiles on, next read after the coming barrier
            run[threadIdx.x] += s;
            wc[par][0][threadIdx.x] = 0; wc[par][1][threadIdx.x] = 0; wc[par][2][threadIdx.x] = 0; wc[par][3][threadIdx.x] = 0;
        }
    }
}

// histogram, scan and placement of one pass on ctx->stream.  hist: rows * plan.blocks words of scratch, 16-byte aligned; total_out
// (optional): the number of elements; start_out (optional): see the placement
template <class POL> static inline hipError_t count_pass(nx_ctx* ctx, const POL& pol, u32 total, CountPlan plan, u32 rows, u32* hist, u32* total_out, u32* start_out) {
    hipLaunchKernelGGL(count_hist_kernel<POL>, dim3(plan.blocks), dim3(CP_THREADS), 0, ctx->stream, pol, total, plan.tiles, rows, hist);
    hipLaunchKernelGGL(scan_kernel<0>, dim3(1), dim3(CP_THREADS), 0, ctx->stream, hist, rows * plan.blocks, total_out);
    hipLaunchKernelGGL(count_place_kernel<POL>, dim3(plan.blocks), dim3(CP_THREADS), 0, ctx->stream, pol, total, plan.tiles, rows, (const u32*)hist, start_out);
    return hipGetLastError();
}
