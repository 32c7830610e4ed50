// Host-side self-test of nexus-zkvm_amd/csrc/host/narrow_pack.h, the pack / check routine of the narrow host-trace upload
// (NX_COL_U32_AS_U8 / NX_COL_U32_AS_U16): packed bytes against a scalar narrowing, and the refusal — the lowest (column, row) whose value
// does not fit — the same under 1, 3 and 16 threads.  Boundary values 0, 255, 256, 65535, 65536, P - 1 and random data, sizes from 2
// words up (across the task size PACK_BLOCK).  Built by tests/test_narrow_upload_cpu.py with hipcc (no GPU needed).  Exit code 0 = all pass.
#include "../../nexus-zkvm_amd/csrc/host/narrow_pack.h"
#include <stdio.h>
#include <random>
using namespace nx;
static const uint32_t P = 0x7fffffffu;
static unsigned long long n_checks = 0, n_bad = 0;
#define CHECK(cond, ...) do { n_checks++; if (!(cond)) { n_bad++; printf("FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

// one case: n_cols columns of n values with the given widths; returns the refusal of the 1-thread run (or none)
static void run_case(const std::vector<std::vector<uint32_t>>& cols, const std::vector<uint8_t>& width, uint64_t n, const char* name) {
    const uint32_t nc = (uint32_t)cols.size();
    // expected: scalar narrowing, first violation in (column, row) order
    PackViolation want;
    for (uint32_t c = 0; c < nc && !want.found; c++)
        for (uint64_t r = 0; r < n; r++) if (cols[c][r] > (width[c] == 1 ? 255u : 65535u)) { want.found = true; want.col = c; want.row = r; want.value = cols[c][r]; break; }
    for (int threads : {1, 3, 16}) {
        std::vector<std::vector<uint8_t>> out(nc);
        std::vector<const uint32_t*> src(nc); std::vector<uint8_t*> dst(nc);
        for (uint32_t c = 0; c < nc; c++) { out[c].assign(n * width[c] + 16, 0xa5); src[c] = cols[c].data(); dst[c] = out[c].data(); }
        PackViolation got;
        const bool ok = pack_narrow(src.data(), dst.data(), width.data(), nc, n, threads, &got);
        CHECK(ok == !want.found, "%s threads %d: verdict %d, expected %d", name, threads, (int)ok, (int)!want.found);
        if (!ok && want.found)
            CHECK(got.col == want.col && got.row == want.row && got.value == want.value, "%s threads %d: refused (%u, %llu, %u), expected (%u, %llu, %u)", name, threads,
                  got.col, (unsigned long long)got.row, got.value, want.col, (unsigned long long)want.row, want.value);
        if (ok) {
            bool same = true;
            for (uint32_t c = 0; c < nc; c++) {
                for (uint64_t r = 0; r < n && same; r++) {
                    const uint32_t v = width[c] == 1 ? out[c][r] : (uint32_t)out[c][2 * r] | (uint32_t)out[c][2 * r + 1] << 8;
                    same = v == cols[c][r];
                }
                for (size_t b = n * width[c]; b < out[c].size(); b++) same = same && out[c][b] == 0xa5;      // nothing written past the column
            }
            CHECK(same, "%s threads %d: packed bytes differ", name, threads);
        }
    }
}

int main() {
    std::mt19937_64 rng(7);
    const uint32_t edge[] = {0u, 255u, 256u, 65535u, 65536u, P - 1};
    for (uint64_t n : {(uint64_t)2, (uint64_t)4, (uint64_t)16, (uint64_t)1000, PACK_BLOCK + 3, 3 * PACK_BLOCK}) {
        for (int nc : {1, 5, 16}) {
            std::vector<uint8_t> width(nc);
            for (int c = 0; c < nc; c++) width[c] = (uint8_t)(1 + (c % 2));
            // random data that fits its width
            std::vector<std::vector<uint32_t>> cols(nc, std::vector<uint32_t>(n));
            for (int c = 0; c < nc; c++) for (auto& v : cols[c]) v = (uint32_t)(rng() & (width[c] == 1 ? 0xffu : 0xffffu));
            char name[96];
            snprintf(name, sizeof name, "random n=%llu cols=%d", (unsigned long long)n, nc);
            run_case(cols, width, n, name);
            // every boundary value at a random row of a random column (the rest fits): fits or is refused at that spot
            for (uint32_t e : edge) {
                auto c2 = cols;
                const int c = (int)(rng() % nc); const uint64_t r = rng() % n;
                c2[c][r] = e;
                snprintf(name, sizeof name, "edge %u at (%d, %llu) n=%llu cols=%d", e, c, (unsigned long long)r, (unsigned long long)n, nc);
                run_case(c2, width, n, name);
            }
            // several violations in several columns: the lowest column, then row, whatever the thread count
            if (nc > 2) {
                auto c3 = cols;
                c3[nc - 1][0] = P - 1; c3[nc / 2][n - 1] = 70000; c3[nc / 2][n / 2] = 65536 + (uint32_t)(n & 7); c3[1][n - 1] = 1u << 20;
                snprintf(name, sizeof name, "several violations n=%llu cols=%d", (unsigned long long)n, nc);
                run_case(c3, width, n, name);
            }
        }
    }
    printf("%llu checks, %llu mismatches\n", n_checks, n_bad);
    return n_bad ? 1 : 0;
}
