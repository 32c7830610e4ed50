// host shim for csrc/prev_access.hip: runs its kernels on the CPU, a block as 256 lock-step threads in 4 waves of 64 with ballot and
// shuffle, LDS as static storage.  Same face as tests/native/mult_emul/internal.h, another engine: the sort kernels vote nine times per
// 256 elements, and a vote between 64 operating-system threads costs milliseconds, so here the 256 threads of a block are fibers
// (ucontext) of ONE thread, resumed in turn; a barrier is a counter and a generation number.  The sanitizers are told about every
// stack switch.
#pragma once
#include <cstdint>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <string>
#include <vector>
#include <algorithm>
#include <functional>
#include <ucontext.h>
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/common_interface_defs.h>
#endif
#include "nexus_hip.h"
typedef uint32_t u32; typedef uint64_t u64;
constexpr u32 P = 0x7fffffffu;
struct uint4 { u32 x, y, z, w; };
inline uint4 make_uint4(u32 a, u32 b, u32 c, u32 d) { return {a, b, c, d}; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
inline dim3 threadIdx, blockIdx, blockDim, gridDim;       // of the fiber that runs: set at every resume
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
#define NX_HD inline
using std::min; using std::max;

namespace emu {
constexpr int N = 256; constexpr size_t STACK = 48 << 10;     // the sanitizer clears a stack's shadow at every switch: no larger than the kernels need
enum { RUNNING, DONE };
struct Fiber { ucontext_t uc; char* stack; int state; };
inline Fiber fib[N]; inline ucontext_t main_uc; inline int cur;
inline const void* main_bottom; inline size_t main_size;
inline const std::function<void()>* body;
inline u32 wave_arrived[4], wave_gen[4], block_arrived, block_gen;
inline u64 xch[2][4][64]; inline u32 xch_turn[N];
inline void to_main(bool dying) {
#if defined(__SANITIZE_ADDRESS__)
    void* fake = nullptr;
    __sanitizer_start_switch_fiber(dying ? nullptr : &fake, main_bottom, main_size);
#endif
    swapcontext(&fib[cur].uc, &main_uc);
#if defined(__SANITIZE_ADDRESS__)
    __sanitizer_finish_switch_fiber(fake, &main_bottom, &main_size);
#endif
}
inline void entry() {
#if defined(__SANITIZE_ADDRESS__)
    __sanitizer_finish_switch_fiber(nullptr, &main_bottom, &main_size);
#endif
    (*body)();
    fib[cur].state = DONE;
    to_main(true);
}
inline void wave_barrier() {
    const int w = threadIdx.x >> 6; const u32 gen = wave_gen[w];
    if (++wave_arrived[w] == 64) { wave_arrived[w] = 0; wave_gen[w]++; return; }
    while (wave_gen[w] == gen) to_main(false);
}
inline void block_barrier() {
    const u32 gen = block_gen;
    if (++block_arrived == (u32)N) { block_arrived = 0; block_gen++; return; }
    while (block_gen == gen) to_main(false);
}
// every lane puts a word up, one barrier, every lane reads; two sets of words taken in turn, so the next exchange cannot overwrite
// what a slower lane has yet to read (it is at most one barrier behind)
template <class T> inline T wave_read(T v, int src) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63; const u32 turn = xch_turn[threadIdx.x]++ & 1;
    u64 raw = 0; memcpy(&raw, &v, sizeof(T)); xch[turn][w][l] = raw;
    wave_barrier();
    T r; memcpy(&r, &xch[turn][w][src & 63], sizeof(T));
    return r;
}
inline void launch(dim3 grid, dim3 block, const std::function<void()>& f) {
    if (block.x != (unsigned)N) { fprintf(stderr, "emu: 256-thread blocks only\n"); abort(); }
    gridDim = grid; blockDim = block; body = &f;
    for (unsigned b = 0; b < grid.x; b++) {
        blockIdx = dim3(b);
        memset(wave_arrived, 0, sizeof wave_arrived); block_arrived = 0; memset(xch_turn, 0, sizeof xch_turn);
        for (int t = 0; t < N; t++) {
            if (!fib[t].stack) fib[t].stack = (char*)aligned_alloc(4096, STACK);      // kept: a test program
            getcontext(&fib[t].uc);
            fib[t].uc.uc_stack.ss_sp = fib[t].stack; fib[t].uc.uc_stack.ss_size = STACK; fib[t].uc.uc_link = nullptr;
            makecontext(&fib[t].uc, entry, 0);
            fib[t].state = RUNNING;
        }
        for (int left = N; left;) {
            left = 0;
            for (int t = 0; t < N; t++) {
                if (fib[t].state == DONE) continue;
                cur = t; threadIdx = dim3(t);
#if defined(__SANITIZE_ADDRESS__)
                void* fake = nullptr;
                __sanitizer_start_switch_fiber(&fake, fib[t].stack, STACK);
#endif
                swapcontext(&main_uc, &fib[t].uc);
#if defined(__SANITIZE_ADDRESS__)
                __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
                if (fib[t].state != DONE) left++;
            }
        }
    }
}
}  // namespace emu

inline void __syncthreads() { emu::block_barrier(); }
inline u64 __ballot(int p) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63; const u32 turn = emu::xch_turn[threadIdx.x]++ & 1;
    emu::xch[turn][w][l] = p ? 1 : 0;
    emu::wave_barrier();
    u64 m = 0; for (int i = 0; i < 64; i++) m |= (emu::xch[turn][w][i] & 1) << i;
    return m;
}
template <class T> inline T __shfl(T v, int lane, int) { return emu::wave_read(v, lane); }
inline int __popcll(u64 x) { return __builtin_popcountll(x); }
inline u32 bitrev(u32 i, int log) { u32 r = 0; for (int b = 0; b < log; b++) r |= ((i >> b) & 1u) << (log - 1 - b); return r; }
inline u32 atomicAdd(u32* p, u32 v) { const u32 o = *p; *p = o + v; return o; }       // one fiber runs at a time
template <class T> inline T atomicMin(T* p, T v) { const T o = *p; if (v < o) *p = v; return o; }
inline u32 gld(const u32* p) { return *p; }
inline uint4 gld4(const u32* p) { if ((uintptr_t)p & 15) { fprintf(stderr, "misaligned gld4\n"); abort(); } return {p[0], p[1], p[2], p[3]}; }
inline uint4 gld4_guarded(const u32* col, u32 row, u32 n, bool vec) {
    if (vec) return gld4(col + row);
    const auto at = [&](u32 i) { return i < n ? col[i] : 0u; };
    return {at(row), at(row + 1), at(row + 2), at(row + 3)};
}
struct PackedKey { u32 n_cols, bits[4], shift[4], total_bits; };
inline void gst(u32* p, u32 v) { *p = v; }
inline void gst4(u32* p, uint4 v) { if ((uintptr_t)p & 15) { fprintf(stderr, "misaligned gst4\n"); abort(); } p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }

typedef int hipError_t; constexpr hipError_t hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
struct nx_ctx { int n_cus = 3; void* stream = nullptr; std::string err; size_t live = 0, live_bytes = 0, peak_bytes = 0; };
namespace nx {
inline int set_err(nx_ctx* c, int code, const std::string& m) { if (c) c->err = m; else fprintf(stderr, "[null ctx] %s\n", m.c_str()); return code; }
inline int hip_fail(nx_ctx* c, hipError_t, const char* w, const char*, int) { return set_err(c, NX_ERR_HIP, w); }
struct DeviceGuard { explicit DeviceGuard(const nx_ctx*) {} };
#define NX_GUARD(c) nx::DeviceGuard nx_guard__(c)
#define NX_TRY(call) do { int rc__ = (call); if (rc__ != NX_OK) return rc__; } while (0)
// an allocation is exactly as long as asked (not rounded up), so that the sanitizer sees the first word past its end
// and it never comes zeroed or with a previous owner's plausible words: dev_alloc fills it with 0xA5A5A5A5 (>= p, nonzero), dev_free with
// 0xFFFFFFFF before the memory goes back
inline void fill_bytes(void* p, size_t bytes, u32 w) { for (size_t i = 0; i < bytes; i++) ((unsigned char*)p)[i] = (unsigned char)(w >> (8 * (i & 3))); }
inline int dev_alloc(nx_ctx* c, size_t bytes, void** out) {
    size_t* p = (size_t*)malloc(bytes + 256); p[0] = bytes; *out = (char*)p + 256;
    fill_bytes(*out, bytes, 0xA5A5A5A5u);
    c->live++; c->live_bytes += bytes; c->peak_bytes = std::max(c->peak_bytes, c->live_bytes); return NX_OK;
}
inline void dev_free(nx_ctx* c, void* p) { size_t* q = (size_t*)((char*)p - 256); c->live--; c->live_bytes -= q[0]; fill_bytes(p, q[0], 0xFFFFFFFFu); free(q); }
inline int upload_async_staged(nx_ctx*, void* d, const void* h, size_t n) { memcpy(d, h, n); return NX_OK; }
inline int copy_d2h_blocking(nx_ctx*, void* h, const void* d, size_t n) { memcpy(h, d, n); return NX_OK; }
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu::launch((g), (b), [=]() { k(__VA_ARGS__); })
}  // namespace nx
