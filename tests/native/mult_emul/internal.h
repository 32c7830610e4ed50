// host shim: runs the kernels of multiplicity.hip on CPU threads in lock step (256 threads per block, 4 waves of 64)
#pragma once
#include <cstdint>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <string>
#include <vector>
#include <algorithm>
#include <barrier>
#include <thread>
#include <functional>
#include <memory>
#include "nexus_hip.h"
typedef uint32_t u32; typedef uint64_t u64;
constexpr u32 P = 0x7fffffffu;
struct uint4 { u32 x, y, z, w; };
inline uint4 make_uint4(u32 a, u32 b, u32 c, u32 d) { return {a, b, c, d}; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
inline thread_local dim3 threadIdx, blockIdx;
inline dim3 blockDim, gridDim;
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
using std::min; using std::max;

inline std::barrier<>* g_block_bar; inline std::barrier<>* g_wave_bar[4];
inline u64 g_xch[4][64];
inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
template <class T> inline T wave_read(T v, int src) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    u64 raw = 0; memcpy(&raw, &v, sizeof(T)); g_xch[w][l] = raw;
    g_wave_bar[w]->arrive_and_wait();
    T r; memcpy(&r, &g_xch[w][src & 63], sizeof(T));
    g_wave_bar[w]->arrive_and_wait();
    return r;
}
inline u64 __ballot(int p) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = p ? 1 : 0;
    g_wave_bar[w]->arrive_and_wait();
    u64 m = 0; for (int i = 0; i < 64; i++) m |= (u64)(g_xch[w][i] & 1) << i;
    g_wave_bar[w]->arrive_and_wait();
    return m;
}
inline int __all(int p) { return __ballot(p) == ~(u64)0; }
inline int nx_ffsll(unsigned long long x) { return __builtin_ffsll((long long)x); }
#define __ffsll nx_ffsll
template <class T> inline T __shfl(T v, int lane, int) { return wave_read(v, lane); }
template <class T> inline T __shfl_xor(T v, int mask, int) { return wave_read(v, (int)(threadIdx.x & 63) ^ mask); }
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline unsigned long long atomicExch(unsigned long long* p, unsigned long long v) { return __atomic_exchange_n(p, v, __ATOMIC_RELAXED); }
template <class T> inline T atomicMin(T* p, T v) { T o = __atomic_load_n(p, __ATOMIC_RELAXED); while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} return o; }
inline u32 gld(const u32* p) { return *p; }
inline uint4 gld4(const u32* p) { if ((uintptr_t)p & 15) { fprintf(stderr, "misaligned gld4\n"); abort(); } return {p[0], p[1], p[2], p[3]}; }
inline uint4 gld4_guarded(const u32* col, u32 row, u32 n, bool vec) {
    if (vec) return gld4(col + row);
    const auto at = [&](u32 i) { return i < n ? col[i] : 0u; };
    return {at(row), at(row + 1), at(row + 2), at(row + 3)};
}
struct PackedKey { u32 n_cols, bits[4], shift[4], total_bits; };
inline void gst(u32* p, u32 v) { *p = v; }

typedef int hipError_t; constexpr hipError_t hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipMemsetAsync(void* p, int v, size_t n, void*) { memset(p, v, n); return 0; }
struct nx_ctx { int n_cus = 3; void* stream = nullptr; std::string err; size_t live = 0; };
namespace nx {
inline int set_err(nx_ctx* c, int code, const std::string& m) { if (c) c->err = m; else fprintf(stderr, "[null ctx] %s\n", m.c_str()); return code; }
inline int hip_fail(nx_ctx* c, hipError_t, const char* w, const char*, int) { return set_err(c, NX_ERR_HIP, w); }
struct DeviceGuard { explicit DeviceGuard(const nx_ctx*) {} };
#define NX_GUARD(c) nx::DeviceGuard nx_guard__(c)
#define NX_TRY(call) do { int rc__ = (call); if (rc__ != NX_OK) return rc__; } while (0)
struct ColSet { uint32_t* base; uint64_t stride; uint32_t* const* table; uint32_t* col(uint32_t c) const { return table ? table[c] : base + (uint64_t)c * stride; } };
inline int make_colset(nx_ctx*, const uint32_t* const* h, uint32_t n, ColSet* out) {
    out->base = nullptr; out->stride = 0;
    uint32_t** t = (uint32_t**)malloc(sizeof(void*) * (n + 1));      // leaked: a test program
    for (uint32_t i = 0; i < n; i++) t[i] = (uint32_t*)h[i];
    out->table = t; return NX_OK;
}
// A block never comes zeroed or with a previous owner's plausible words: dev_alloc fills the whole rounded block with 0xA5A5A5A5 (>= p,
// nonzero), dev_free with 0xFFFFFFFF before the memory goes back.  The rounded size sits in a 256-byte header in front of the block.
inline void fill_words(void* p, size_t bytes, u32 w) { for (size_t i = 0; i < bytes / 4; i++) ((u32*)p)[i] = w; }
inline int dev_alloc(nx_ctx* c, size_t bytes, void** out) {
    const size_t rounded = (std::max<size_t>(bytes, 4) + 255) & ~(size_t)255;
    char* q = (char*)aligned_alloc(256, 256 + rounded); *(size_t*)q = rounded; *out = q + 256;
    fill_words(*out, rounded, 0xA5A5A5A5u);
    c->live++; return NX_OK;
}
inline void dev_free(nx_ctx* c, void* p) { if (!p) { c->live--; return; } char* q = (char*)p - 256; fill_words(p, *(size_t*)q, 0xFFFFFFFFu); free(q); c->live--; }
inline int upload_async_staged(nx_ctx*, void* d, const void* h, size_t n) { memcpy(d, h, n); return NX_OK; }
inline int copy_d2h_blocking(nx_ctx*, void* h, const void* d, size_t n) { memcpy(h, d, n); return NX_OK; }

inline void emu_launch(dim3 grid, dim3 block, const std::function<void()>& body) {
    if (block.x != 256) { fprintf(stderr, "emu: 256-thread blocks only\n"); abort(); }
    gridDim = grid; blockDim = block;
    std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64), step(256);
    g_block_bar = &bb; g_wave_bar[0] = &w0; g_wave_bar[1] = &w1; g_wave_bar[2] = &w2; g_wave_bar[3] = &w3;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < 256; t++)
        th.emplace_back([&, t] {
            for (unsigned b = 0; b < grid.x; b++) {
                threadIdx = dim3(t); blockIdx = dim3(b);
                body();
                step.arrive_and_wait();          // static "shared" memory is reused by the next block
            }
        });
    for (auto& x : th) x.join();
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) nx::emu_launch((g), (b), [=]() { k(__VA_ARGS__); })
}  // namespace nx
