// The kernel text nx_trace_program generates for programs with 32-bit integer registers (the RV32M chips' fill program and the table of
// the seven W opcodes: tests/rv32m_air.py), run on the host (tests/test_rv32m_cpu.py).
//
// The generated source is header-free C++ apart from two work-item builtins and a few attributes, so a plain C++ compiler builds every
// kernel as an ordinary function once the builtins are given a meaning.  The arithmetic is the text's own: PACK32's truncation, the
// products, the division helpers with their zero-divisor rules.  Every kernel of a segmented program is run over the whole trace, one
// after the other, as they are launched.
//
// Build (the test does): clang++ -x c++ -std=c++17 -fsanitize=address,undefined -DGEN_SRC='"generated.hip"' -DGEN_KERNELS=air_kernel,air_kernel_1
//                        rv32m_text_host.cpp
// Run: rv32m_text_host operands.bin [operands.bin ...]   — per file, u32 words: log_size, n_cols, the columns before the run (2^log_size
// words each, stored order), the columns the model expects afterwards.  EVERY word of every column is compared: an input column and
// a STORE_IF row whose flag is 0 must keep what they held.
// Prints one line per file, "<file>: <rows> rows, <k> mismatches"; exit status 0 only when every count is 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static unsigned g_block, g_lane;
#define __builtin_amdgcn_workgroup_id_x() g_block
#define __builtin_amdgcn_workitem_id_x() g_lane
#define amdgpu_flat_work_group_size(a, b)
#include GEN_SRC

typedef void (*trace_fn)(u32* const*, int, u32);
static const trace_fn kernels[] = {GEN_KERNELS};

static size_t run_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<u32> w;
    u32 buf[4096]; size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    fclose(f);
    if (w.size() < 2 || w[0] < 1 || w[0] > 20 || w.size() != 2 + 2 * ((size_t)w[1] << w[0])) { fprintf(stderr, "%s: malformed operand file\n", path); exit(2); }
    const u32 log_size = w[0], n_cols = w[1], n_rows = 1u << log_size;
    std::vector<std::vector<u32>> cols(n_cols);              // exactly n_rows words each: a store beyond the trace is the sanitizer's
    for (u32 k = 0; k < n_cols; k++) cols[k].assign(w.begin() + 2 + (size_t)k * n_rows, w.begin() + 2 + (size_t)(k + 1) * n_rows);
    std::vector<u32*> ptrs(n_cols);
    for (u32 k = 0; k < n_cols; k++) ptrs[k] = cols[k].data();
    const u32 lanes = (n_rows + 255) / 256 * 256;            // whole blocks, as launched: the lanes beyond the trace must do nothing
    for (const trace_fn fn : kernels)
        for (u32 r = 0; r < lanes; r++) { g_block = r / 256; g_lane = r % 256; fn(ptrs.data(), (int)log_size, n_rows); }
    const u32* want = w.data() + 2 + (size_t)n_cols * n_rows;
    size_t bad = 0;
    for (u32 k = 0; k < n_cols; k++)
        for (u32 r = 0; r < n_rows; r++)
            if (cols[k][r] != want[(size_t)k * n_rows + r]) {
                if (bad < 8) fprintf(stderr, "%s: column %u position %u: got %u, want %u\n", path, k, r, cols[k][r], want[(size_t)k * n_rows + r]);
                bad++;
            }
    printf("%s: %u rows, %zu mismatches\n", path, n_rows, bad);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s operands.bin [operands.bin ...]\n", argv[0]); return 2; }
    size_t bad = 0;
    for (int k = 1; k < argc; k++) bad += run_file(argv[k]);
    return bad ? 1 : 0;
}
