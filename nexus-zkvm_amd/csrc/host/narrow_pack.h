// Host side of the narrow host-trace upload (NX_COL_U32_AS_U16 / NX_COL_U32_AS_U8, include/nexus_hip.h): u32 columns the caller holds
// in the reference's layout (byte limbs stored as u32, prover/src/trace/utils.rs:57-61) are packed to 1 or 2 bytes per value on host
// threads, and every value is checked in the same pass.  Header-only and free of HIP, so tests/native/narrow_pack_selftest.cpp runs it on
// the CPU.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace nx {

// The first value that does not fit its declared width: column (index into the pack's column list) and row (index into that column).
struct PackViolation { bool found = false; uint32_t col = 0; uint64_t row = 0; uint32_t value = 0; };

// Rows of one task: large enough that a task is mostly streaming, small enough to balance 16 threads over a 16-column chunk.
constexpr uint64_t PACK_BLOCK = 1u << 16;

// dst[i] = src[i] narrowed to W bytes for i in [0, n); returns the first i whose value needs more than W bytes, or n.
template <int W> static inline uint64_t pack_block(const uint32_t* __restrict src, uint8_t* __restrict dst, uint64_t n) {
    constexpr uint32_t over = W == 1 ? ~0xffu : ~0xffffu;
    uint32_t acc = 0;
    if (W == 1) for (uint64_t i = 0; i < n; i++) { const uint32_t v = src[i]; acc |= v; dst[i] = (uint8_t)v; }
    else {
        uint16_t* d16 = (uint16_t*)(void*)dst;           // the caller's slot offsets are multiples of 2 bytes
        for (uint64_t i = 0; i < n; i++) { const uint32_t v = src[i]; acc |= v; d16[i] = (uint16_t)v; }
    }
    if (!(acc & over)) return n;
    for (uint64_t i = 0; i < n; i++) if (src[i] & over) return i;
    return n;
}

// Packs n_cols columns of n values: column c from src[c] (uint32) into dst[c] (width[c] = 1 or 2 bytes per value), on n_threads threads
// (the calling thread included).  Returns true when every value fits.  Otherwise *bad holds the lowest column and, within it, the lowest
// row that does not fit — the same answer under every thread count: each task scans its rows in order and stops at its first violation,
// so the lowest violation overall is the first one of the task that holds it, and the tasks' answers are reduced by (column, row).
// The content of dst is unspecified after a refusal.
static inline bool pack_narrow(const uint32_t* const* src, uint8_t* const* dst, const uint8_t* width, uint32_t n_cols, uint64_t n, int n_threads,
                               PackViolation* bad) {
    const uint64_t blocks_per_col = (n + PACK_BLOCK - 1) / PACK_BLOCK, n_tasks = blocks_per_col * n_cols;
    const int t_use = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, n_threads), n_tasks));
    std::vector<PackViolation> found(t_use);
    std::atomic<uint64_t> next{0};
    auto work = [&](int t) {
        PackViolation& mine = found[t];
        for (uint64_t task = next.fetch_add(1); task < n_tasks; task = next.fetch_add(1)) {
            const uint32_t c = (uint32_t)(task / blocks_per_col);
            const uint64_t r0 = (task % blocks_per_col) * PACK_BLOCK, m = std::min(PACK_BLOCK, n - r0);
            const uint64_t i = width[c] == 1 ? pack_block<1>(src[c] + r0, dst[c] + r0, m) : pack_block<2>(src[c] + r0, dst[c] + 2 * r0, m);
            if (i < m && (!mine.found || c < mine.col || (c == mine.col && r0 + i < mine.row))) {
                mine.found = true; mine.col = c; mine.row = r0 + i; mine.value = src[c][r0 + i];
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < t_use; t++) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    PackViolation best;
    for (const PackViolation& v : found)
        if (v.found && (!best.found || v.col < best.col || (v.col == best.col && v.row < best.row))) best = v;
    if (best.found && bad) *bad = best;
    return !best.found;
}

}  // namespace nx
