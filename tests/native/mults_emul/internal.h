// host shim for csrc/multiplicity_sparse.hip: the fiber engine of tests/native/prev_emul/internal.h (the test copies that file next to
// this one as prev_internal.h), which runs a block as 256 lock-step fibers in 4 waves of 64, plus what the count kernels use beyond
// the sort: the wave-wide vote and butterfly, 64-bit counters, the memset of the counters.
#pragma once
#include "prev_internal.h"

inline int __all(int p) { return __ballot(p) == ~(u64)0; }
inline int nx_ffsll(unsigned long long x) { return __builtin_ffsll((long long)x); }
#define __ffsll nx_ffsll
template <class T> inline T __shfl_xor(T v, int mask, int) { return emu::wave_read(v, (int)(threadIdx.x & 63) ^ mask); }
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; *p = o + v; return o; }   // one fiber runs at a time
inline hipError_t hipMemsetAsync(void* p, int v, size_t n, void*) { memset(p, v, n); return 0; }
