// The kernel text nx_air_compile / nx_logup_program generate, run on the host (tests/test_air_text_host_cpu.py).
//
// The generated source is header-free C++ apart from two work-item builtins and a few attributes, so a plain C++ compiler builds every
// kernel as an ordinary function once the builtins are given a meaning: this driver calls it once per row.  The arithmetic is the text's
// own — the AIR_PRELUDE / LOGUP_PRELUDE copies of field.cuh and whatever the generator emitted around them (lazy accumulators of the
// dot-product peephole, the fold schedule of the constraint sum, Montgomery's trick over a group of denominators).
//
// Build (the test does): clang++ -x c++ -std=c++17 -fsanitize=address,undefined -DGEN_SRC='"generated.hip"' -DGEN_KERNELS=air_kernel,air_kernel_1
//                        -DGEN_LOGUP=0|1 air_text_host.cpp
// Run: air_text_host operands.bin   — u32 words: n_rows, log_size, log_eval, n_cols, n_econsts, n_roots, then the columns (n_rows words
// each), the secure constants (4 each) and, for constraint kernels, the alpha powers (4 per constraint), denom_inv (n_rows >> log_size
// words) and the 4 start accumulator columns; then the expected words: 4 accumulator columns, or 4 columns per logup column.
// Prints "<rows> rows, <k> mismatches, <m> words not below p"; exit status 0 only when both counts are 0.
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
typedef void (*cons_fn)(const u32* const*, const u32*, const u32*, const u32*, int, int, u32*, u32*, u32*, u32*, u32, u32);
typedef void (*logup_fn)(const u32* const*, const u32*, u32* const*, int, u32);
#if GEN_LOGUP
const logup_fn kernels[] = {GEN_KERNELS};
#else
const cons_fn kernels[] = {GEN_KERNELS};
#endif

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
    const u32 n_rows = in.one(), log_size = in.one(), log_eval = in.one(), n_cols = in.one(), n_econsts = in.one(), n_roots = in.one();
    std::vector<std::vector<u32>> cols(n_cols);
    for (auto& c : cols) c = in.take(n_rows);
    std::vector<const u32*> col_ptrs(n_cols ? n_cols : 1, nullptr);
    for (u32 k = 0; k < n_cols; k++) col_ptrs[k] = cols[k].data();
    const std::vector<u32> econsts = in.take(4 * (size_t)n_econsts);
    const size_t n_out = GEN_LOGUP ? 4 * (size_t)n_roots : 4;
    std::vector<std::vector<u32>> out(n_out);
#if GEN_LOGUP
    (void)log_eval;
    for (auto& o : out) o.assign(n_rows, 0xffffffffu);
    std::vector<u32*> out_ptrs(n_out);
    for (size_t k = 0; k < n_out; k++) out_ptrs[k] = out[k].data();
    for (const logup_fn fn : kernels)                    // a later kernel starts from the running sum the one before stored: kernel after kernel, as launched
        for (u32 r = 0; r < n_rows; r++) { g_block = r / 256; g_lane = r % 256; fn(col_ptrs.data(), econsts.data(), out_ptrs.data(), (int)log_size, n_rows); }
#else
    const std::vector<u32> pw = in.take(4 * (size_t)n_roots), denom_inv = in.take(n_rows >> log_size);
    for (auto& o : out) o = in.take(n_rows);
    for (const cons_fn fn : kernels)
        for (u32 r = 0; r < n_rows; r++) {
            g_block = r / 256; g_lane = r % 256;
            fn(col_ptrs.data(), econsts.data(), pw.data(), denom_inv.data(), (int)log_size, (int)log_eval, out[0].data(), out[1].data(), out[2].data(), out[3].data(), 0, n_rows);
        }
#endif
    size_t bad = 0, big = 0;
    for (size_t k = 0; k < n_out; k++) {
        const std::vector<u32> want = in.take(n_rows);
        for (u32 r = 0; r < n_rows; r++) {
            if (out[k][r] >= P) big++;
            if (out[k][r] != want[r]) { if (bad < 8) fprintf(stderr, "output %zu row %u: got %u, want %u\n", k, r, out[k][r], want[r]); bad++; }
        }
    }
    if (in.at != in.w.size()) { fprintf(stderr, "operand file has %zu words left over\n", in.w.size() - in.at); return 2; }
    printf("%u rows, %zu mismatches, %zu words not below p\n", n_rows, bad, big);
    return bad || big ? 1 : 0;
}
