// csrc/keccak_memcheck.h — the column emitter nx_trace_keccak_memory_check's kernel compiles, with the round of csrc/keccak_round.h —
// as plain host C++ (tests/test_keccak_memcheck_cpu.py builds it with -fsanitize=address,undefined).  One call of km_fill_row per
// storage position, as the kernel makes it, into columns that are exactly 2^log_size words long, so an index out of its column is the
// sanitizer's to find.
//   keccak_memcheck_host n_instances log_size in.bin out.bin
// in.bin: n_instances x 25 little-endian u64, then n_instances addresses, then n_instances x 200 timestamps (u32 words); out.bin: the
// 2001 main columns, the preprocessed column (u32 words), then the n_instances x 25 output lanes.
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
#include "keccak_memcheck.h"

struct HostStore {
    std::vector<std::vector<u32>>* cols; u32 pos;
    void word(u32 col, u32 w) const { cols->at(col).at(pos) = w; }
    HostStore here() const { return *this; }
    void put(u32 col, u64 lane) const { for (u32 b = 0; b < 8; b++) word(col + b, (u32)(lane >> (8 * b)) & 255u); }
};

// row: the instance's 200 timestamps, exactly; NULL on a padding row
struct HostTimestamps {
    const std::vector<u32>* row;
    void ts4(u32 j, u32 (&w)[4]) const { for (u32 k = 0; k < 4; k++) w[k] = row ? row->at(4 * j + k) : 0; }
};

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: keccak_memcheck_host n_instances log_size in.bin out.bin\n"); return 2; }
    const u32 n_inst = (u32)atoi(argv[1]), log_size = (u32)atoi(argv[2]), n = 1u << log_size;
    std::vector<u64> states((size_t)n_inst * KR_LANES), out((size_t)n_inst * KR_LANES, 0);
    std::vector<u32> addresses(n_inst);
    std::vector<std::vector<u32>> timestamps(n_inst, std::vector<u32>(KM_STATE));
    FILE* f = fopen(argv[3], "rb");
    bool ok = f && (states.empty() || (fread(states.data(), 8, states.size(), f) == states.size() && fread(addresses.data(), 4, n_inst, f) == n_inst));
    for (u32 r = 0; ok && r < n_inst; r++) ok = fread(timestamps[r].data(), 4, KM_STATE, f) == KM_STATE;
    if (!ok) { fprintf(stderr, "cannot read the inputs\n"); return 2; }
    fclose(f);
    std::vector<std::vector<u32>> main_cols(KM_MAIN_COLS, std::vector<u32>(n, 0xDEADBEEFu)), pre_cols(KM_PRE_COLS, std::vector<u32>(n, 0xDEADBEEFu));
    for (u32 pos = 0; pos < n; pos++) {
        const u32 r = coset_row_of_pos(pos, (int)log_size);
        const bool real = r < n_inst;
        u64 a[KR_LANES];
        for (u32 l = 0; l < KR_LANES; l++) a[l] = real ? states.at((size_t)r * KR_LANES + l) : 0;
        const HostStore m{&main_cols, pos}, p{&pre_cols, pos};
        const HostTimestamps ts{real ? &timestamps.at(r) : nullptr};
        km_fill_row(m, p, true, a, real ? addresses.at(r) : 0, ts, !real, r == n - 1);
        if (real) for (u32 l = 0; l < KR_LANES; l++) out.at((size_t)r * KR_LANES + l) = a[l];
    }
    f = fopen(argv[4], "wb");
    if (!f) { fprintf(stderr, "cannot write\n"); return 2; }
    for (const auto& c : main_cols) fwrite(c.data(), 4, n, f);
    for (const auto& c : pre_cols) fwrite(c.data(), 4, n, f);
    if (!out.empty()) fwrite(out.data(), 8, out.size(), f);
    fclose(f);
    return 0;
}
