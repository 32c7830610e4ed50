// csrc/keccak_round.h — the round and the column emitter nx_trace_keccak_round's kernel compiles — as plain host C++
// (tests/test_keccak_round_cpu.py builds it with -fsanitize=address,undefined).  One call of kr_fill_row per storage position, as the
// kernel makes it, into columns that are exactly 2^log_size words long, so an index out of its column is the sanitizer's to find.
//   keccak_round_host n_instances first_round log_rounds log_size states.bin out.bin
// states.bin: n_instances x 25 little-endian u64; out.bin: the 1705 main columns, the 9 preprocessed columns (u32 words), then the
// n_instances x 25 output lanes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef uint32_t u32;
typedef uint64_t u64;
#define NX_HD inline
static inline u32 bitrev(u32 i, int log) { u32 r = 0; for (int b = 0; b < log; b++) r |= ((i >> b) & 1u) << (log - 1 - b); return r; }
#include "trace_rows.h"
#include "keccak_round.h"

struct HostStore {
    std::vector<std::vector<u32>>* cols; u32 pos;
    void word(u32 col, u32 w) const { cols->at(col).at(pos) = w; }
    void put(u32 col, u64 lane) const { for (u32 b = 0; b < 8; b++) word(col + b, (u32)(lane >> (8 * b)) & 255u); }
};

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: keccak_round_host n_instances first_round log_rounds log_size states.bin out.bin\n"); return 2; }
    const u32 n_inst = (u32)atoi(argv[1]), first = (u32)atoi(argv[2]), log_rounds = (u32)atoi(argv[3]), log_size = (u32)atoi(argv[4]);
    const u32 rounds = 1u << log_rounds, n = 1u << log_size;
    std::vector<u64> states((size_t)n_inst * KR_LANES), out((size_t)n_inst * KR_LANES, 0);
    FILE* f = fopen(argv[5], "rb");
    if (!f || (!states.empty() && fread(states.data(), 8, states.size(), f) != states.size())) { fprintf(stderr, "cannot read the states\n"); return 2; }
    fclose(f);
    std::vector<std::vector<u32>> main_cols(KR_MAIN_COLS, std::vector<u32>(n, 0xDEADBEEFu)), pre_cols(KR_PRE_COLS, std::vector<u32>(n, 0xDEADBEEFu));
    for (u32 pos = 0; pos < n; pos++) {
        const u32 r = coset_row_of_pos(pos, (int)log_size), i = r & (rounds - 1), inst = r >> log_rounds;
        const bool real = inst < n_inst;
        u64 a[KR_LANES];
        for (u32 l = 0; l < KR_LANES; l++) a[l] = real ? states.at((size_t)inst * KR_LANES + l) : 0;
        const HostStore m{&main_cols, pos}, p{&pre_cols, pos};
        kr_fill_row(m, p, true, a, i, first, rounds, !real, r == n - 1);
        if (real && i == rounds - 1) for (u32 l = 0; l < KR_LANES; l++) out.at((size_t)inst * KR_LANES + l) = a[l];
    }
    f = fopen(argv[6], "wb");
    if (!f) { fprintf(stderr, "cannot write\n"); return 2; }
    for (const auto& c : main_cols) fwrite(c.data(), 4, n, f);
    for (const auto& c : pre_cols) fwrite(c.data(), 4, n, f);
    if (!out.empty()) fwrite(out.data(), 8, out.size(), f);
    fclose(f);
    return 0;
}
