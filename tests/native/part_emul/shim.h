// What csrc/trace_partition.hip needs on the host beyond tests/native/prev_emul/internal.h (the lock-step engine: 256 fibers per block,
// waves of 64 with ballot and shuffle): the constant-address-space reads and SGPR-base stores of the fill kernel as plain loads and
// stores, and the context's staging ring as exact-size heap blocks, so that the sanitizer sees the first byte past a descriptor table.
#pragma once
#include <memory>
#define NX_TP_HOST_SHIM 1
#include "internal.h"
namespace nx {
template <class T> inline T tp_uniform(const T* p) { return *p; }
inline u32 tp_load(const u32* base, u32 byte_off) { return *(const u32*)((const char*)base + byte_off); }
inline void tp_store(u32* base, u32 byte_off, u32 w) { *(u32*)((char*)base + byte_off) = w; }
inline u32 tp_here(u32 off) { return off; }
inline std::vector<void*> staged_blocks;
inline int stage(nx_ctx*, const void* h, size_t bytes, void** d) { void* p = malloc(bytes ? bytes : 1); memcpy(p, h, bytes); staged_blocks.push_back(p); *d = p; return NX_OK; }
inline void staged_release() { for (void* p : staged_blocks) free(p); staged_blocks.clear(); }
#define NX_LAUNCH_CHECK(ctx) do { } while (0)
}  // namespace nx
