// The kernel text nx_trace_program generates, run on the host (tests/test_trace_program_cpu.py).
//
// The generated source is header-free C++ apart from two work-item builtins and a few attributes (tests/native/air_text_host.cpp), so a
// plain C++ compiler builds every kernel as an ordinary function once the builtins are given a meaning: this driver calls every kernel
// once per storage position, kernel after kernel, as they are launched.  The arithmetic is the text's own: the integer opcodes and their
// reduction (TRACE_PRELUDE), the M31 inverse, the natural-row mapping of the loads and of ROW.
//
// Build (the test does): clang++ -x c++ -std=c++17 -fsanitize=address,undefined -DGEN_SRC='"generated.hip"' -DGEN_KERNELS=air_kernel,air_kernel_1
//                        trace_text_host.cpp
// Run: trace_text_host operands.bin   — u32 words: n_rows, log_size, n_cols, then the columns as they are before the run (n_rows words
// each, stored order), then the same columns as they must be afterwards: EVERY column is compared, so a word the program must not
// touch (an input column, a STORE_IF row whose flag is 0) is checked too.
// Prints "<rows> rows, <k> mismatches, <m> stored words not below p"; exit status 0 only when both counts are 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static unsigned g_block, g_lane;
#define __builtin_amdgcn_workgroup_id_x() g_block
#define __builtin_amdgcn_workitem_id_x() g_lane
#define amdgpu_flat_work_group_size(a, b)
#include GEN_SRC

namespace {
typedef void (*trace_fn)(u32* const*, int, u32);
const trace_fn kernels[] = {GEN_KERNELS};

struct Reader {
    std::vector<u32> w; size_t at = 0;
    u32 one() { if (at >= w.size()) { fprintf(stderr, "operand file too short\n"); exit(2); } return w[at++]; }
    std::vector<u32> take(size_t n) { if (n > w.size() - at) { fprintf(stderr, "operand file too short\n"); exit(2); } std::vector<u32> v(w.begin() + at, w.begin() + at + n); at += n; return v; }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s operands.bin\n", argv[0]); return 2; }
    Reader in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        u32 buf[4096]; size_t got;
        while ((got = fread(buf, 4, 4096, f)) > 0) in.w.insert(in.w.end(), buf, buf + got);
        fclose(f);
    }
    const u32 n_rows = in.one(), log_size = in.one(), n_cols = in.one();
    if (n_rows != 1u << log_size) { fprintf(stderr, "n_rows is not 2^log_size\n"); return 2; }
    std::vector<std::vector<u32>> cols(n_cols);              // exactly n_rows words each: a store beyond the trace is the sanitizer's
    for (auto& c : cols) c = in.take(n_rows);
    const std::vector<std::vector<u32>> before = cols;
    std::vector<u32*> ptrs(n_cols ? n_cols : 1, nullptr);
    for (u32 k = 0; k < n_cols; k++) ptrs[k] = cols[k].data();
    const u32 lanes = (n_rows + 255) / 256 * 256;            // whole blocks, as launched: the lanes beyond the trace must do nothing
    for (const trace_fn fn : kernels)
        for (u32 r = 0; r < lanes; r++) { g_block = r / 256; g_lane = r % 256; fn(ptrs.data(), (int)log_size, n_rows); }
    size_t bad = 0, big = 0;
    for (u32 k = 0; k < n_cols; k++) {
        const std::vector<u32> want = in.take(n_rows);
        for (u32 r = 0; r < n_rows; r++) {
            if (cols[k][r] != before[k][r] && cols[k][r] >= P) big++;
            if (cols[k][r] != want[r]) { if (bad < 8) fprintf(stderr, "column %u position %u: got %u, want %u\n", k, r, cols[k][r], want[r]); bad++; }
        }
    }
    if (in.at != in.w.size()) { fprintf(stderr, "operand file has %zu words left over\n", in.w.size() - in.at); return 2; }
    printf("%u rows, %zu mismatches, %zu stored words not below p\n", n_rows, bad, big);
    return bad || big ? 1 : 0;
}
