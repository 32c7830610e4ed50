// nx_logup_multiplicities_sparse on the host: csrc/multiplicity_sparse.hip compiled as plain C++ against tests/native/mults_emul/internal.h,
// which runs a block as 256 fibers in lock step (waves of 64 with ballot / shuffle, LDS as static storage), so the entry point with
// its sort passes, its check, its two-level search, its scatter and its second walk is compared with a count over a std::map — under
// the address and undefined-behaviour sanitizers, which watch every splitter, segment, counter and position index.  Built twice: as
// it is, and with -DNX_COUNT_PASS_MAX_BLOCKS=2 -DNX_MULT_SPARSE_LDS_LOG_KEYS=1, where a block of the sort takes many tiles and every
// table of more than two rows is searched in global memory behind two splitters.
#include "multiplicity_sparse_emu.cpp"   // a copy of csrc/multiplicity_sparse.hip next to the shim internal.h (the test makes it)
#include <random>
#include <map>
#include <set>

static std::mt19937_64 rng(4242);
typedef std::vector<u32> Bits;
struct Use { std::vector<std::vector<u32>> cols; std::vector<u32> w; bool has_w; u32 log; };
struct Table { std::vector<std::vector<u32>> cols; std::vector<u32> valid; bool has_valid; u32 log; std::vector<u64> keys; };   // keys: of the valid rows
static std::vector<u32*> g_allocs;
static u32* dup_aligned(const std::vector<u32>& v, size_t misalign_words = 0) {
    // exactly as long as the column, so that the sanitizer sees the first word past its end (malloc gives 16-byte alignment)
    u32* p = (u32*)malloc(std::max<size_t>(4, (v.size() + misalign_words) * 4));
    u32* q = p + misalign_words;
    if (!v.empty()) memcpy(q, v.data(), v.size() * 4);
    g_allocs.push_back(p);
    return q;
}
static u32 total_bits(const Bits& b) { u32 t = 0; for (u32 x : b) t += x; return t; }
static u64 key_of(const Bits& bits, const std::vector<std::vector<u32>>& cols, size_t r, bool* ok) {
    u64 key = 0; u32 sh = 0; *ok = true;
    for (size_t c = 0; c < bits.size(); c++) { const u64 x = cols[c][r]; if (x >> bits[c]) *ok = false; key |= (x & (((u64)1 << bits[c]) - 1)) << sh; sh += bits[c]; }
    return key;
}
static void put_key(const Bits& bits, std::vector<std::vector<u32>>& cols, size_t r, u64 key) {
    u32 sh = 0;
    for (size_t c = 0; c < bits.size(); c++) { cols[c][r] = (u32)((key >> sh) & (((u64)1 << bits[c]) - 1)); sh += bits[c]; }
}
// mode 0: every row valid (as far as the key space has keys), 1: half, 2: one, 3: none.  spread 0: random keys, 1: keys that share
// their top 24 bits (where there are that many), 2: 0 and the largest key among them
static Table make_table(const Bits& bits, u32 log, int mode, int spread) {
    Table t; t.log = log; const size_t n = (size_t)1 << log; const u32 tb = total_bits(bits);
    const u64 space = (u64)1 << tb;
    size_t want = mode == 0 ? n : mode == 1 ? (n + 1) / 2 : mode == 2 ? 1 : 0;
    if (want > space) want = (size_t)space;
    if (spread == 1 && tb > 8 && want > 200) want = 200;
    std::set<u64> ks;
    if (spread == 2 && want >= 2) { ks.insert(0); ks.insert(space - 1); }
    const u64 top = rng() & (space - 1) & ~(u64)255;
    while (ks.size() < want) ks.insert(spread == 1 && tb > 8 ? top | (rng() & 255) : rng() & (space - 1));
    t.keys.assign(ks.begin(), ks.end());
    std::vector<size_t> where(n); for (size_t i = 0; i < n; i++) where[i] = i;
    std::shuffle(where.begin(), where.end(), rng);
    std::vector<u64> order(t.keys); std::shuffle(order.begin(), order.end(), rng);
    t.cols.assign(bits.size(), std::vector<u32>(n, 0)); t.valid.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        const size_t r = where[i];
        if (i < want) { put_key(bits, t.cols, r, order[i]); t.valid[r] = 1 + (u32)(rng() % 5) * 1000; continue; }
        // no table row: a copy of a valid key, or anything, values outside their bits included
        if (want && (rng() & 1)) put_key(bits, t.cols, r, order[rng() % want]);
        else for (auto& c : t.cols) c[r] = (u32)rng();
    }
    t.has_valid = want != n;
    return t;
}
// dist 0: keys of the table, now and then a neighbour; 1: one key of the table; 2: mostly the smallest key; 3: anything
static Use make_use(const Bits& bits, const Table& t, u32 log, int dist, int wmode) {
    Use u; u.log = log; u.has_w = wmode != 0; const size_t n = (size_t)1 << log; const u32 tb = total_bits(bits); const u64 space = (u64)1 << tb;
    u.cols.assign(bits.size(), std::vector<u32>(n, 0));
    const u64 one = t.keys.empty() ? 0 : t.keys[rng() % t.keys.size()];
    for (size_t r = 0; r < n; r++) {
        u64 key;
        if (t.keys.empty() || dist == 3) key = rng() & (space - 1);
        else if (dist == 1) key = one;
        else if (dist == 2) key = rng() % 10 ? t.keys[0] : t.keys[rng() % t.keys.size()];
        else { key = t.keys[rng() % t.keys.size()]; if (rng() % 64 == 0) key = (key + (rng() & 1 ? 1 : space - 1)) & (space - 1); }
        put_key(bits, u.cols, r, key);
    }
    const u32 ws[4] = {0, 1, P - 1, P - 2};
    u.w.resize(n); for (auto& x : u.w) x = wmode == 1 ? rng() & 1 : wmode == 2 ? P - 1 : ws[rng() & 3];
    return u;
}
static int n_fail = 0;
static u64 mem_bound(u32 log_table, size_t n_uses) {
    const u64 T = (u64)1 << log_table;
    return 16 * T + 1024 * std::min<u64>(256, (T + 1023) / 1024) + 52 * n_uses + 4 * MS_LDS_KEYS + 4096;
}
static void run_case(const char* name, const Bits& bits, const Table& t, std::vector<Use>& uses, int expect_rc, size_t misalign = 0, const char* expect_text = nullptr) {
    const u32 k = (u32)bits.size();
    // reference
    std::map<u64, size_t> row_of; bool table_ok = true;
    for (size_t p = 0; p < t.cols[0].size(); p++) {
        if (t.has_valid && !t.valid[p]) continue;
        bool ok; const u64 key = key_of(bits, t.cols, p, &ok);
        if (!ok || row_of.count(key)) table_ok = false; else row_of[key] = p;
    }
    std::vector<unsigned __int128> sum(t.cols[0].size(), 0);
    u64 n_missing = 0, first = ~(u64)0;
    for (size_t u = 0; u < uses.size(); u++)
        for (size_t r = 0; r < ((size_t)1 << uses[u].log); r++) {
            const u32 w = uses[u].has_w ? uses[u].w[r] : 1; if (!w) continue;
            bool ok; const u64 key = key_of(bits, uses[u].cols, r, &ok);
            const auto it = ok ? row_of.find(key) : row_of.end();
            if (it != row_of.end()) sum[it->second] += w;
            else { n_missing++; first = std::min<u64>(first, ((u64)u << 32) | r); }
        }
    // call
    nx_ctx ctx;
    std::vector<std::vector<const u32*>> ptrs(uses.size()); std::vector<nx_lookup_use> lu(uses.size());
    for (size_t u = 0; u < uses.size(); u++) {
        for (u32 c = 0; c < k; c++) ptrs[u].push_back(dup_aligned(uses[u].cols[c], misalign));
        lu[u].d_values = ptrs[u].data(); lu[u].d_weight = uses[u].has_w ? dup_aligned(uses[u].w, misalign) : nullptr; lu[u].log_size = uses[u].log;
    }
    std::vector<const u32*> tp; for (u32 c = 0; c < k; c++) tp.push_back(dup_aligned(t.cols[c], misalign));
    const u32* valid = t.has_valid ? dup_aligned(t.valid, misalign) : nullptr;
    u32* mult = dup_aligned(std::vector<u32>(t.cols[0].size(), 0xDEADBEEF), misalign);
    u64 nm = 99; u32 fu = 99; u64 fp = 99;
    const int rc = nx_logup_multiplicities_sparse(&ctx, lu.data(), (u32)uses.size(), k, bits.data(), tp.data(), valid, t.log, mult, &nm, &fu, &fp);
    bool ok = rc == expect_rc && ctx.live == 0 && ctx.live_bytes == 0 && (rc == NX_ERR_ARG) == !table_ok;
    if (ctx.peak_bytes > mem_bound(t.log, uses.size())) { ok = false; printf("  peak %zu above the bound %llu\n", ctx.peak_bytes, (unsigned long long)mem_bound(t.log, uses.size())); }
    if (rc != NX_ERR_ARG) {
        for (size_t p = 0; p < sum.size(); p++) if (mult[p] != (u32)(sum[p] % P)) { ok = false; printf("  pos %zu: got %u want %u\n", p, mult[p], (u32)(sum[p] % P)); break; }
        if (nm != n_missing) ok = false;
        if (n_missing && (fu != (u32)(first >> 32) || fp != (first & 0xFFFFFFFFu))) ok = false;
    }
    if (expect_text && ctx.err.find(expect_text) == std::string::npos) ok = false;
    printf("%-44s rc %d (want %d) missing %llu (want %llu) first (%u,%llu) %s  %s\n", name, rc, expect_rc, (unsigned long long)nm, (unsigned long long)n_missing, fu, (unsigned long long)fp,
           ok ? "OK" : "FAIL", rc ? ctx.err.c_str() : "");
    if (!ok) n_fail++;
    for (u32* p : g_allocs) free(p);
    g_allocs.clear();
}
static int expect_of(const Bits& bits, const Table& t, const std::vector<Use>& uses) {
    std::set<u64> ks(t.keys.begin(), t.keys.end());
    for (auto& u : uses)
        for (size_t r = 0; r < ((size_t)1 << u.log); r++) {
            if (u.has_w && !u.w[r]) continue;
            bool ok; const u64 key = key_of(bits, u.cols, r, &ok);
            if (!ok || !ks.count(key)) return NX_ERR_PROTOCOL;
        }
    return NX_OK;
}
int main() {
    printf("block cap %u\nLDS keys %u\n", (unsigned)CP_MAX_BLOCKS, (unsigned)MS_LDS_KEYS);
    const std::vector<Bits> keyings = {{32}, {16, 16}, {8, 8, 8, 8}, {20}, {1}, {3, 2, 4, 5}};
    const u32 big = std::max<u32>(12, std::min<u32>(MS_LDS_LOG_KEYS + 1, 13));   // as built: the first table the LDS does not hold whole; 2^12 rows: eight tiles per block under a cap of 2
    bool two_level = false, many_tiles = false;
    for (auto& bits : keyings) {
        const u32 tb = total_bits(bits);
        const u32 logs_t[] = {0, 1, 2, 6, 8, 10, big};
        int v = 0;
        for (u32 lt : logs_t) {
            for (int mode = 0; mode < 4; mode++, v++) {
                if (lt >= 10 && mode >= 2 && bits.size() != 2) continue;              // the large tables: not every combination
                if (lt == big && (mode >= 2 || bits.size() > 2)) continue;
                Table t = make_table(bits, lt, mode, v % 3);
                std::vector<Use> uses;
                const u32 logs[] = {0, 1, 2, 6, 12, 2, 13};
                for (int i = 0; i < (lt >= 8 ? 7 : 5); i++) uses.push_back(make_use(bits, t, logs[i], (i + v) % 4, (i + mode) % 4));
                char nm[80]; snprintf(nm, 80, "bits %u cols %zu table 2^%u mode %d", tb, bits.size(), lt, mode);
                run_case(nm, bits, t, uses, expect_of(bits, t, uses));
                if (lt > MS_LDS_LOG_KEYS && t.keys.size() > MS_LDS_KEYS) two_level = true;
                if (ms_count_plan((u64)1 << lt).tiles > CP_MIN_TILES) many_tiles = true;
                if (mode == 1 && (lt == 2 || lt == big)) { snprintf(nm, 80, "bits %u table 2^%u misaligned columns", tb, lt); run_case(nm, bits, t, uses, expect_of(bits, t, uses), 1 + v % 3); }
            }
        }
        // heavy: p - 1 on one key over 2^12 rows; no use at all
        { Table t = make_table(bits, 6, 1, 0); std::vector<Use> uses{make_use(bits, t, 12, 1, 2)}; run_case("  all p-1 on one key", bits, t, uses, NX_OK); }
        { Table t = make_table(bits, 6, 1, 0); std::vector<Use> none; run_case("  no uses", bits, t, none, NX_OK); }
        // missing rows: out of range and absent; an entry out of range under weight 0
        if (tb < 32 || bits.size() > 1) {
            Table t = make_table(bits, 8, 0, 0);
            std::vector<Use> uses{make_use(bits, t, 6, 1, 0), make_use(bits, t, 13, 1, 0), make_use(bits, t, 3, 1, 0)};
            u32 c = 0; while (bits[c] == 32) c++;
            uses[1].cols[c][4321] = 1u << bits[c]; uses[2].cols[c][5] = 0xFFFFFFFFu;
            run_case("  two out of range", bits, t, uses, NX_ERR_PROTOCOL, 0, "use 1 row position 4321");
            uses[1].has_w = true; uses[1].w.assign((size_t)1 << 13, 1); uses[1].w[4321] = 0; uses[2].cols[c][5] = uses[2].cols[c][4];
            run_case("  out of range under weight 0", bits, t, uses, NX_OK);
        }
        if (tb >= 8) {   // keys just below the smallest, just above the largest and between two neighbours
            Table t = make_table(bits, 6, 0, 1);
            std::vector<u64> absent;
            if (t.keys.front() > 0) absent.push_back(t.keys.front() - 1);
            if (t.keys.back() + 1 < ((u64)1 << tb)) absent.push_back(t.keys.back() + 1);
            for (size_t i = 0; i + 1 < t.keys.size(); i++) if (t.keys[i + 1] - t.keys[i] > 1) { absent.push_back(t.keys[i] + 1); break; }
            std::vector<Use> uses{make_use(bits, t, 7, 1, 0), make_use(bits, t, 7, 1, 0)};
            for (size_t i = 0; i < absent.size(); i++) put_key(bits, uses[1].cols, 100 - 10 * i, absent[i]);
            run_case("  absent neighbours", bits, t, uses, absent.empty() ? NX_OK : NX_ERR_PROTOCOL, 0, absent.empty() ? nullptr : "is not a row of the table");
        }
        if (tb >= 4) {
            { Table t = make_table(bits, 4, 0, 0); for (auto& c : t.cols) c[9] = c[3]; std::vector<Use> uses{make_use(bits, t, 5, 0, 0)};
              run_case("  duplicate table key", bits, t, uses, NX_ERR_ARG, 0, "table row positions 3 and 9 hold the same key"); }
            { Table t = make_table(bits, 4, 1, 0); size_t a = 0; while (!t.valid[a]) a++; size_t b = a + 1; while (b < 16 && t.valid[b]) b++;
              if (b < 16) for (auto& c : t.cols) c[b] = c[a]; std::vector<Use> uses{make_use(bits, t, 5, 0, 0)};
              run_case("  a copy of a key in a row that is none", bits, t, uses, expect_of(bits, t, uses)); }
        }
        if (tb < 32 || bits.size() > 1) {
            Table t = make_table(bits, 4, 0, 0); u32 c = 0; while (bits[c] == 32) c++;
            t.cols[c][5] = 1u << bits[c]; std::vector<Use> uses{make_use(bits, t, 5, 0, 0)};
            if (t.keys.size() == 16) run_case("  table value out of range", bits, t, uses, NX_ERR_ARG, 0, "table row position 5 holds a value outside its key_bits");
        }
    }
    {   // refusals decided on the host
        nx_ctx ctx; u32 bits1[1] = {33}, bits2[2] = {16, 17}, bits0[1] = {0}, okb[1] = {8};
        u32 col[4] = {1, 2, 3, 4}, out[4]; const u32* tp[1] = {col}; const u32* alias[1] = {out};
        const u32* uv[1] = {col}; nx_lookup_use lu = {uv, nullptr, 2};
        int bad = 0;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 1, bits1, tp, nullptr, 2, out, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 2, bits2, tp, nullptr, 2, out, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 1, bits0, tp, nullptr, 2, out, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 0, okb, tp, nullptr, 2, out, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 5, okb, tp, nullptr, 2, out, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 1, okb, tp, nullptr, 31, out, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 1, okb, alias, nullptr, 2, out, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 1, okb, tp, out, 2, out, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 1, okb, tp, nullptr, 2, col, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, nullptr, 1, 1, okb, tp, nullptr, 2, out, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 1, okb, tp, nullptr, 2, nullptr, nullptr, nullptr, nullptr) != NX_ERR_ARG;
        bad += ctx.live != 0;
        bad += nx_logup_multiplicities_sparse(&ctx, &lu, 1, 1, okb, tp, nullptr, 2, out, nullptr, nullptr, nullptr) != NX_OK || out[0] != 1 || out[3] != 1;
        printf("%-44s %s\n", "host-side refusals, then a good call", bad ? "FAIL" : "OK ");
        n_fail += bad != 0;
    }
    if (!two_level) { printf("PLAN NOT REACHED: no table was searched in two levels\n"); n_fail++; }
    if (CP_MAX_BLOCKS < 1024 && !many_tiles) { printf("PLAN NOT REACHED: no block of the sort took more than %u tiles\n", CP_MIN_TILES); n_fail++; }
    printf("%d failures\n", n_fail);
    return n_fail != 0;
}
