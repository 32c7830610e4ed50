// nx_logup_multiplicities on the host: csrc/multiplicity.hip compiled as plain C++ against tests/native/mult_emul/internal.h, which runs a
// block as 256 threads in lock step (waves of 64 with ballot / shuffle, LDS as static storage, atomics as host atomics), so the entry
// point with its four kernels is checked against a brute-force count — under the address and undefined-behaviour sanitizers.
#include "multiplicity_emu.cpp"   // a copy of csrc/multiplicity.hip next to the shim internal.h (the test makes it)
#include <random>
#include <map>

static std::mt19937_64 rng(12345);
struct Use { std::vector<std::vector<u32>> cols; std::vector<u32> w; bool has_w; u32 log; };
static u32* dup_aligned(const std::vector<u32>& v, size_t misalign_words = 0) {
    u32* p = (u32*)aligned_alloc(256, ((v.size() + misalign_words) * 4 + 255) & ~(size_t)255);
    memcpy(p + misalign_words, v.data(), v.size() * 4); return p + misalign_words;
}
static int n_fail = 0;
static void run_case(const char* name, const std::vector<u32>& bits, const std::vector<std::vector<u32>>& table, u32 log_table, std::vector<Use>& uses, int expect_rc, size_t misalign = 0) {
    const u32 k = bits.size(); u32 tb = 0; std::vector<u32> sh(k); for (u32 c = 0; c < k; c++) { sh[c] = tb; tb += bits[c]; }
    // reference
    std::vector<u64> cnt((size_t)1 << tb, 0); std::vector<char> present((size_t)1 << tb, 0);
    std::vector<u32> tkey((size_t)1 << log_table);
    for (size_t p = 0; p < tkey.size(); p++) { u32 key = 0; for (u32 c = 0; c < k; c++) key |= table[c][p] << sh[c]; tkey[p] = key; if (expect_rc != NX_ERR_ARG) present[key] = 1; }
    u64 n_missing = 0, first = ~(u64)0;
    for (size_t u = 0; u < uses.size(); u++)
        for (size_t r = 0; r < ((size_t)1 << uses[u].log); r++) {
            const u32 w = uses[u].has_w ? uses[u].w[r] : 1; if (!w) continue;
            bool ok = true; u32 key = 0;
            for (u32 c = 0; c < k; c++) { const u32 x = uses[u].cols[c][r]; if (x >> bits[c]) ok = false; else key |= x << sh[c]; }
            if (ok) cnt[key] += w;
            if (!ok || (expect_rc != NX_ERR_ARG && !present[key])) { n_missing++; first = std::min<u64>(first, ((u64)u << 32) | r); }
        }
    // call
    nx_ctx ctx;
    std::vector<std::vector<const u32*>> ptrs(uses.size()); std::vector<nx_lookup_use> lu(uses.size());
    for (size_t u = 0; u < uses.size(); u++) {
        for (u32 c = 0; c < k; c++) ptrs[u].push_back(dup_aligned(uses[u].cols[c], misalign));
        lu[u].d_values = ptrs[u].data(); lu[u].d_weight = uses[u].has_w ? dup_aligned(uses[u].w, misalign) : nullptr; lu[u].log_size = uses[u].log;
    }
    std::vector<const u32*> tp; for (u32 c = 0; c < k; c++) tp.push_back(dup_aligned(table[c]));
    std::vector<u32> mult((size_t)1 << log_table, 0xDEADBEEF);
    u64 nm = 99; u32 fu = 99; u64 fp = 99;
    const int rc = nx_logup_multiplicities(&ctx, lu.data(), (u32)uses.size(), k, bits.data(), tp.data(), log_table, mult.data(), &nm, &fu, &fp);
    bool ok = rc == expect_rc && ctx.live == 0;
    if (rc != NX_ERR_ARG) {
        for (size_t p = 0; p < tkey.size(); p++) if (mult[p] != (u32)(cnt[tkey[p]] % P)) { ok = false; printf("  pos %zu: got %u want %u\n", p, mult[p], (u32)(cnt[tkey[p]] % P)); break; }
        if (nm != n_missing) ok = false;
        if (n_missing && (fu != (u32)(first >> 32) || fp != (first & 0xFFFFFFFFu))) ok = false;
    }
    printf("%-40s rc %d (want %d) missing %llu (want %llu) first (%u,%llu) %s  %s\n", name, rc, expect_rc, (unsigned long long)nm, (unsigned long long)n_missing, fu, (unsigned long long)fp,
           ok ? "OK" : "FAIL", rc ? ctx.err.c_str() : "");
    if (!ok) n_fail++;
}
static std::vector<std::vector<u32>> table_of(const std::vector<u32>& bits, u32 log_table, int order) {
    std::vector<u32> keys((size_t)1 << log_table); for (size_t i = 0; i < keys.size(); i++) keys[i] = (u32)i;
    if (order == 1) std::reverse(keys.begin(), keys.end());
    if (order == 2) std::shuffle(keys.begin(), keys.end(), rng);
    std::vector<std::vector<u32>> t(bits.size()); u32 sh = 0;
    for (size_t c = 0; c < bits.size(); c++) { for (u32 key : keys) t[c].push_back((key >> sh) & ((1u << bits[c]) - 1)); sh += bits[c]; }
    return t;
}
static Use make_use(const std::vector<u32>& bits, u32 log, int dist, int wmode) {
    Use u; u.log = log; u.has_w = wmode != 0; const size_t n = (size_t)1 << log;
    for (u32 b : bits) { std::vector<u32> c(n); for (auto& x : c) x = dist == 0 ? rng() % (1u << b) : dist == 1 ? 0 : (rng() % 10 ? 0 : rng() % (1u << b)); u.cols.push_back(c); }
    if (dist == 3) for (auto& c : u.cols) { std::fill(c.begin(), c.end(), 0); c[n / 2] = 1; }
    const u32 ws[4] = {0, 1, P - 1, P - 2};
    u.w.resize(n); for (auto& x : u.w) x = wmode == 1 ? rng() & 1 : wmode == 2 ? P - 1 : ws[rng() & 3];
    return u;
}
int main() {
    const std::vector<std::vector<u32>> keyings = {{4}, {8}, {12}, {13}, {8, 8}, {3, 2, 4, 5}};
    for (auto& bits : keyings) {
        u32 tb = 0; for (u32 b : bits) tb += b;
        for (int order = 0; order < 3; order++) {
            auto t = table_of(bits, tb, order);
            std::vector<Use> uses;
            const u32 logs[] = {0, 3, 6, 12, 13, 2, 14};
            for (int i = 0; i < 7; i++) uses.push_back(make_use(bits, logs[i], (i + order) % 4, i % 4));
            char nm[64]; snprintf(nm, 64, "bits %u order %d", tb, order);
            run_case(nm, bits, t, tb, uses, NX_OK);
            if (order == 0) { snprintf(nm, 64, "bits %u misaligned columns", tb); run_case(nm, bits, t, tb, uses, NX_OK, 1); }
        }
        // heavy: p-1 on one key over 2^12 rows
        { auto t = table_of(bits, tb, 2); std::vector<Use> uses{make_use(bits, 12, 1, 2)}; run_case("  all p-1 on one key", bits, t, tb, uses, NX_OK); }
        // missing rows: out of range and absent
        {
            auto t = table_of(bits, tb, 2);
            std::vector<Use> uses{make_use(bits, 6, 0, 0), make_use(bits, 13, 0, 0), make_use(bits, 3, 0, 0)};
            uses[1].cols[0][4321] = 1u << bits[0]; uses[2].cols[0][5] = P - 1;
            run_case("  two out of range", bits, t, tb, uses, NX_ERR_PROTOCOL);
            uses[1].has_w = true; uses[1].w.assign((size_t)1 << 13, 1); uses[1].w[4321] = 0; uses[2].cols[0][5] = 0;
            run_case("  out of range under weight 0", bits, t, tb, uses, NX_OK);
        }
        if (tb >= 4) {   // a table with only even keys, half the rows
            auto full = table_of(bits, tb, 0);
            std::vector<std::vector<u32>> t(bits.size());
            for (size_t c = 0; c < bits.size(); c++) for (size_t p = 0; p < full[c].size(); p += 2) t[c].push_back(full[c][p]);
            std::vector<Use> uses{make_use(bits, 11, 0, 0)};
            for (auto& x : uses[0].cols[0]) x &= ~1u;
            uses[0].cols[0][1500] |= 1; uses[0].cols[0][7] |= 1;
            run_case("  absent odd keys", bits, t, tb - 1, uses, NX_ERR_PROTOCOL);
        }
        { auto t = table_of(bits, tb, 0); for (size_t c = 0; c < bits.size(); c++) t[c][3] = t[c][9]; std::vector<Use> uses{make_use(bits, 5, 0, 0)}; run_case("  duplicate table key", bits, t, tb, uses, NX_ERR_ARG); }
        { auto t = table_of(bits, tb, 0); t[0][5] = 1u << bits[0]; std::vector<Use> uses{make_use(bits, 5, 0, 0)}; run_case("  table value out of range", bits, t, tb, uses, NX_ERR_ARG); }
    }
    { std::vector<u32> bits{4}; auto t = table_of(bits, 4, 0); std::vector<Use> none; run_case("no uses", bits, t, 4, none, NX_OK); }
    printf("%d failures\n", n_fail);
    return n_fail != 0;
}
