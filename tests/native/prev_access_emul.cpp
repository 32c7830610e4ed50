// nx_trace_prev_access on the host: csrc/prev_access.hip (with csrc/access_history.cuh) compiled as plain C++ against tests/native/prev_emul/internal.h (256 lock-step
// threads per block as fibers, waves of 64 with ballot / shuffle, LDS as static storage), so the entry point with its kernels is checked
// against a sequential walk over a map — under the address and undefined-behaviour sanitizers, which watch every LDS, histogram and
// placement index.  Built twice by the test: as it is, and with -DNX_COUNT_PASS_MAX_BLOCKS=2, where a block of the sort takes more tiles
// than the minimum.
#include "prev_access_emu.cpp"   // a copy of csrc/prev_access.hip next to the shim internal.h, access_history.cuh, trace_rows.h and count_pass.cuh (the test makes it)
#include <random>
#include <map>

static std::mt19937_64 rng(20251);
static int n_fail = 0, n_ok = 0;

struct Stream {
    std::vector<std::vector<u32>> key, pay;      // pay[c] empty: a NULL payload column
    std::vector<u32> flag; bool has_flag = false;
    std::vector<char> prev_wanted;               // per payload column; empty: d_prev == NULL
    bool want_ord = true;
    u32 log = 0, epoch = 0, linear = 0;
};
static u32* dup_aligned(const std::vector<u32>& v, size_t misalign_words = 0) {
    u32* p = (u32*)aligned_alloc(256, ((v.size() + misalign_words) * 4 + 255) & ~(size_t)255);
    memcpy(p + misalign_words, v.data(), v.size() * 4); return p + misalign_words;
}
// the model's own row of a storage position, from the definition: position = bitrev(index in the circle domain), the domain holds
// the even coset rows in its first half and the odd ones, backwards, in its second
static u32 model_row_of_pos(u32 pos, u32 log) {
    u32 d = 0; for (u32 b = 0; b < log; b++) d |= ((pos >> b) & 1u) << (log - 1 - b);
    const u32 n = 1u << log;
    return d < n / 2 ? 2 * d : 2 * (n - 1 - d) + 1;
}
struct Want { std::vector<std::vector<std::vector<u32>>> prev; std::vector<std::vector<u32>> ord; std::vector<u32> skey, scount; std::vector<std::vector<u32>> slast; u64 first_bad = ~(u64)0; };
static Want model(const std::vector<Stream>& st, const std::vector<u32>& bits, u32 np, const std::vector<u32>& init) {
    struct Acc { u32 epoch, row, s, pos; };
    std::vector<Acc> acc;
    for (u32 s = 0; s < st.size(); s++)
        for (u32 pos = 0; pos < (1u << st[s].log); pos++) acc.push_back({st[s].epoch, st[s].linear ? pos : model_row_of_pos(pos, st[s].log), s, pos});
    std::sort(acc.begin(), acc.end(), [](const Acc& a, const Acc& b) { return std::tie(a.epoch, a.row, a.s) < std::tie(b.epoch, b.row, b.s); });
    Want w; w.prev.resize(st.size()); w.ord.resize(st.size());
    for (u32 s = 0; s < st.size(); s++) { w.prev[s].assign(np, std::vector<u32>((size_t)1 << st[s].log, 0)); w.ord[s].assign((size_t)1 << st[s].log, 0); }
    struct Last { std::vector<u32> pay; u32 count; };
    std::map<u32, Last> last;
    for (const Acc& a : acc) {
        const Stream& S = st[a.s];
        if (S.has_flag && !S.flag[a.pos]) continue;
        u32 key = 0, sh = 0; bool bad = false;
        for (size_t c = 0; c < bits.size(); c++) { const u32 x = S.key[c][a.pos]; if (bits[c] < 32 && (x >> bits[c])) bad = true; key |= x << sh; sh += bits[c]; }
        if (bad) { w.first_bad = std::min<u64>(w.first_bad, ((u64)a.s << 32) | a.pos); continue; }
        auto it = last.find(key);
        for (u32 c = 0; c < np; c++) w.prev[a.s][c][a.pos] = it == last.end() ? init[c] : it->second.pay[c];
        w.ord[a.s][a.pos] = it == last.end() ? 0 : it->second.count;
        Last& l = last[key];
        l.pay.resize(np); for (u32 c = 0; c < np; c++) l.pay[c] = S.pay[c].empty() ? 0 : S.pay[c][a.pos];
        l.count++;
    }
    w.slast.resize(np);
    for (auto& kv : last) { w.skey.push_back(kv.first); w.scount.push_back(kv.second.count); for (u32 c = 0; c < np; c++) w.slast[c].push_back(kv.second.pay[c]); }
    return w;
}

static const u32 GUARD = 0xDEADBEEFu;
// cap: capacity of the summary (~0u: as many as there are keys; the arrays get 4 guard words behind them either way); with_summary 0: none
static void run_case(const char* name, std::vector<Stream>& st, const std::vector<u32>& bits, u32 np, const std::vector<u32>& init, bool with_summary, u32 cap, int expect_rc,
                     size_t misalign = 0) {
    const Want w = model(st, bits, np, init);
    nx_ctx ctx;
    const u32 k = bits.size(), ns = st.size();
    std::vector<std::vector<const u32*>> kp(ns), pp(ns); std::vector<std::vector<u32*>> vp(ns); std::vector<u32*> op(ns, nullptr);
    std::vector<nx_access_stream> as(ns);
    for (u32 s = 0; s < ns; s++) {
        const size_t n = (size_t)1 << st[s].log;
        for (u32 c = 0; c < k; c++) kp[s].push_back(dup_aligned(st[s].key[c], misalign));
        for (u32 c = 0; c < np; c++) pp[s].push_back(st[s].pay[c].empty() ? nullptr : dup_aligned(st[s].pay[c], misalign));
        for (u32 c = 0; c < np && !st[s].prev_wanted.empty(); c++) vp[s].push_back(st[s].prev_wanted[c] ? dup_aligned(std::vector<u32>(n, GUARD), misalign) : nullptr);
        if (st[s].want_ord) op[s] = dup_aligned(std::vector<u32>(n, GUARD), misalign);
        as[s].d_key = kp[s].data(); as[s].d_flag = st[s].has_flag ? dup_aligned(st[s].flag, misalign) : nullptr; as[s].d_payload = pp[s].data();
        as[s].d_prev = st[s].prev_wanted.empty() ? nullptr : vp[s].data(); as[s].d_ordinal = op[s];
        as[s].log_size = st[s].log; as[s].epoch = st[s].epoch; as[s].linear = st[s].linear;
    }
    const u32 nk = (u32)w.skey.size(), real_cap = cap == ~0u ? nk : cap;
    nx_access_summary sum; std::vector<u32*> lastp;
    sum.cap = real_cap; sum.d_key = dup_aligned(std::vector<u32>(real_cap + 4, GUARD)); sum.d_count = dup_aligned(std::vector<u32>(real_cap + 4, GUARD));
    for (u32 c = 0; c < np; c++) lastp.push_back(dup_aligned(std::vector<u32>(real_cap + 4, GUARD)));
    sum.d_last = lastp.data();
    u64 got_keys = 99;
    const int rc = nx_trace_prev_access(&ctx, as.data(), ns, k, bits.data(), np, init.data(), with_summary ? &sum : nullptr, &got_keys);
    bool ok = rc == expect_rc && ctx.live == 0 && ctx.live_bytes == 0;
    std::string why;
    u64 rows = 0; for (u32 s = 0; s < ns; s++) rows += (u64)1 << st[s].log;
    if (ctx.peak_bytes > 18 * rows + 1024 * (u64)ns + 65536) { ok = false; why = "peak of " + std::to_string(ctx.peak_bytes) + " bytes above the documented bound"; }
    if (rc == NX_OK) {
        for (u32 s = 0; s < ns && ok; s++) {
            const size_t n = (size_t)1 << st[s].log;
            for (size_t p = 0; p < n && ok; p++) {
                if (op[s] && op[s][p] != w.ord[s][p]) { ok = false; why = "ordinal of stream " + std::to_string(s) + " pos " + std::to_string(p) + ": " + std::to_string(op[s][p]) + " want " + std::to_string(w.ord[s][p]); }
                for (u32 c = 0; c < np && ok && !st[s].prev_wanted.empty(); c++)
                    if (vp[s][c] && vp[s][c][p] != w.prev[s][c][p]) { ok = false; why = "prev " + std::to_string(c) + " of stream " + std::to_string(s) + " pos " + std::to_string(p) + ": " + std::to_string(vp[s][c][p]) + " want " + std::to_string(w.prev[s][c][p]); }
            }
        }
        if (got_keys != nk) { ok = false; why = "n_keys " + std::to_string(got_keys) + " want " + std::to_string(nk); }
        for (u32 i = 0; i < real_cap + 4 && ok; i++) {
            const bool in = with_summary && i < std::min(real_cap, nk);
            if (sum.d_key[i] != (in ? w.skey[i] : GUARD) || sum.d_count[i] != (in ? w.scount[i] : GUARD)) { ok = false; why = "summary entry " + std::to_string(i); }
            for (u32 c = 0; c < np && ok; c++) if (lastp[c][i] != (in ? w.slast[c][i] : GUARD)) { ok = false; why = "summary last " + std::to_string(c) + " entry " + std::to_string(i); }
        }
    } else if (rc == NX_ERR_PROTOCOL) {
        const std::string at = "stream " + std::to_string((u32)(w.first_bad >> 32)) + " row position " + std::to_string(w.first_bad & 0xFFFFFFFFu) + ":";
        if (w.first_bad == ~(u64)0 || ctx.err.find(at) == std::string::npos) { ok = false; why = "message does not name " + at; }
        if (got_keys != 99) { ok = false; why = "n_keys written on an error"; }
    }
    printf("%-58s rc %d (want %d) keys %llu %s  %s %s\n", name, rc, expect_rc, (unsigned long long)got_keys, ok ? "OK" : "FAIL", why.c_str(), rc ? ctx.err.c_str() : "");
    ok ? n_ok++ : n_fail++;
}

// dist 0: uniform keys; 1: one key; 2: all keys distinct (needs enough bits); 3: mostly zero limbs
static Stream make_stream(const std::vector<u32>& bits, u32 log, u32 np, int dist, bool flags, u32 null_mask, u32 distinct_base = 0) {
    Stream S; S.log = log; const size_t n = (size_t)1 << log;
    u32 tb = 0; for (u32 b : bits) tb += b;
    S.key.assign(bits.size(), std::vector<u32>(n));
    for (size_t p = 0; p < n; p++) {
        u64 key = dist == 0 ? rng() : dist == 1 ? 0x5A5A5A5Au : dist == 2 ? distinct_base + p : (rng() % 8 ? 0 : rng());
        if (dist == 0 && tb > 8) key &= (rng() & 1) ? ~(u64)0 : (u64)((0xFFu << (tb - 8)) | 3u);     // repeats also in wide key spaces
        u32 sh = 0;
        for (size_t c = 0; c < bits.size(); c++) { S.key[c][p] = std::min<u32>(P - 1, (u32)((key >> sh) & (((u64)1 << bits[c]) - 1))); sh += bits[c]; }
    }
    S.pay.resize(np);
    for (u32 c = 0; c < np; c++) { if ((null_mask >> c) & 1) continue; S.pay[c].resize(n); for (auto& x : S.pay[c]) x = dist == 3 && (c & 1) ? 0 : (u32)(rng() % P); }
    S.has_flag = flags; S.flag.resize(n); for (auto& x : S.flag) x = (rng() % 3) ? (u32)(1 + rng() % 5) : 0;
    S.prev_wanted.assign(np, 1); for (u32 c = 0; c < np; c++) if ((null_mask >> (c + 3)) & 1) S.prev_wanted[c] = 0;
    return S;
}

int main() {
    const std::vector<std::vector<u32>> keyings = {{5}, {8, 5}, {8, 8, 8, 8}, {31}};
    const u32 logs[] = {1, 2, 6, 8, 11, 12}, nps[] = {1, 5, 8, 16}, nstr[] = {1, 3, 4};
    int variant = 0;
    for (auto& bits : keyings)
        for (u32 log : logs) {
            // the sizes of more than one block with three streams, the small ones with every stream count
            for (u32 ns : nstr) {
                if (log >= 8 && ns != 3) continue;
                if (log == 12 && (bits.size() == 2 || bits[0] == 31)) continue;      // 2^12 rows: one and five passes
                const u32 np = nps[variant % 4]; const bool flags = variant & 1, with_sum = (variant >> 1) & 1;
                std::vector<u32> init(np); for (auto& x : init) x = (u32)(rng() % P);
                std::vector<Stream> st;
                for (u32 s = 0; s < ns; s++) { st.push_back(make_stream(bits, log, np, 0, flags, variant % 3 == 0 ? 0x12u << s : 0)); st.back().want_ord = (variant + s) % 3 != 0; }
                char nm[96]; snprintf(nm, 96, "bits %zu cols log %u streams %u payload %u flags %d sum %d", bits.size(), log, ns, np, (int)flags, (int)with_sum);
                run_case(nm, st, bits, np, init, with_sum, ~0u, NX_OK, variant % 5 == 4 ? 1 : 0);
                variant++;
            }
        }
    for (auto& bits : keyings) {
        u32 tb = 0; for (u32 b : bits) tb += b;
        const std::vector<u32> init{P - 1, 7, 0, P - 2, 1};
        {   // the chain is the whole trace
            std::vector<Stream> st; for (u32 s = 0; s < 3; s++) st.push_back(make_stream(bits, 9, 5, 1, false, 0));
            run_case("  every access on one key", st, bits, 5, init, true, ~0u, NX_OK);
        }
        if (tb >= 13) {   // every access takes init
            std::vector<Stream> st; for (u32 s = 0; s < 3; s++) st.push_back(make_stream(bits, 9, 5, 2, false, 0, s << 9));
            run_case("  all keys distinct", st, bits, 5, init, true, ~0u, NX_OK);
        }
        {
            std::vector<Stream> st; for (u32 s = 0; s < 4; s++) st.push_back(make_stream(bits, 9, 5, 3, s & 1, 0));
            run_case("  half the columns zero", st, bits, 5, init, true, ~0u, NX_OK);
        }
        {   // a linear image of epoch 0 without outputs, four streams of epoch 1, one more of another size in epoch 1, one in epoch 7
            std::vector<Stream> st;
            st.push_back(make_stream(bits, 7, 5, tb >= 13 ? 2 : 0, false, 0)); st[0].linear = 1; st[0].epoch = 0; st[0].prev_wanted.clear(); st[0].want_ord = false;
            for (u32 s = 0; s < 4; s++) { st.push_back(make_stream(bits, 10, 5, 3, s == 2, 0)); st.back().epoch = 1; }
            for (size_t p = 0; p < 1024; p++)    // touches of imaged addresses
                if (rng() & 1) { const size_t s = 1 + rng() % 4, src = rng() % 128; for (size_t c = 0; c < bits.size(); c++) st[s].key[c][p] = st[0].key[c][src]; }
            st.push_back(make_stream(bits, 6, 5, 0, true, 0)); st.back().epoch = 1;
            st.push_back(make_stream(bits, 0, 5, 1, false, 0)); st.back().epoch = 1; st.back().linear = 1;
            st.push_back(make_stream(bits, 3, 5, 0, false, 0)); st.back().epoch = 7;
            run_case("  epochs and mixed sizes", st, bits, 5, init, true, ~0u, NX_OK);
            run_case("  the same with a summary of 3 entries", st, bits, 5, init, true, 3, NX_OK);
            run_case("  the same with a summary of 0 entries", st, bits, 5, init, true, 0, NX_OK);
        }
        if (bits[0] < 31) {   // an entry out of its bits: refused on an accessing row, ignored on another
            std::vector<Stream> st; for (u32 s = 0; s < 3; s++) st.push_back(make_stream(bits, 9, 5, 0, s != 0, 0));
            st[1].key[0][300] = 1u << bits[0]; st[1].flag[300] = 0; st[2].key[0][77] = P - 1; st[2].flag[77] = 0;
            run_case("  out of range on rows that do not access", st, bits, 5, init, true, ~0u, NX_OK);
            st[2].flag[77] = 1; st[2].key[0][500] = 1u << bits[0]; st[2].flag[500] = 3; st[0].key[0][5] = 0; st[1].flag[300] = 1;
            run_case("  out of range on three accessing rows", st, bits, 5, init, true, ~0u, NX_ERR_PROTOCOL);
            st[0].key[0][511] = P - 1;
            run_case("  and in the stream without flags", st, bits, 5, init, false, ~0u, NX_ERR_PROTOCOL);
        }
    }
    for (const std::vector<u32>& bits : std::vector<std::vector<u32>>{{8}, {8, 8, 8, 8}}) {
        // No flag anywhere and whole-byte keys: the last pass has no digit to spare, so a refused row (key 0, no handle) takes digit 255
        // like the real keys with top byte 255 and stands among them by its lower bytes, then by time.  Key 255 << (bits - 8) has the
        // same lower bytes (none, or zeros), so in time order K, refused, K, refused, K is also their sorted order: the resolve meets
        // elements without a handle with real ones on both sides.
        const std::vector<u32> init{P - 1, 7, 0, P - 2, 1};
        std::vector<Stream> st; for (u32 s = 0; s < 3; s++) st.push_back(make_stream(bits, 9, 5, 0, false, 0));
        const auto pos_of_row = [](u32 row) { u32 pos = 0; while (model_row_of_pos(pos, 9) != row) pos++; return pos; };
        const auto put = [&](u32 s, u32 row, bool refused) {
            const u32 pos = pos_of_row(row);
            for (size_t c = 0; c < bits.size(); c++) st[s].key[c][pos] = !refused && c + 1 == bits.size() ? 255u : 0u;
            if (refused) st[s].key[0][pos] = 256;       // a word of 9 bits in a column of 8
        };
        put(0, 10, false); put(1, 20, true); put(2, 30, false); put(0, 40, true); put(1, 50, false);
        run_case(bits.size() == 1 ? "  refused rows between keys of digit 255, one pass" : "  refused rows between keys of digit 255, four passes", st, bits, 5, init, true, ~0u,
                 NX_ERR_PROTOCOL);
    }
    {   // 2^11 + 2 elements: with a block cap of 2 (the test's second build) a sort block takes five tiles, one more than the minimum, in
        // every one of the two passes (13 key bits and flags); as built it is two blocks of four tiles and one of one
        const std::vector<u32> bits{8, 5}, init{P - 3};
        std::vector<Stream> st;
        st.push_back(make_stream(bits, 11, 1, 0, true, 0)); st.back().linear = 1;
        st.push_back(make_stream(bits, 1, 1, 0, false, 0)); st.back().linear = 1;
        const CountPlan plan = count_plan(((u64)1 << 11) + 2);
        const bool reached = CP_MAX_BLOCKS != 2 || (plan.tiles > CP_MIN_TILES && plan.blocks == 2);
        run_case(reached ? "  linear streams of 2^11 and 2 rows" : "  linear streams of 2^11 and 2 rows: PLAN NOT REACHED", st, bits, 1, init, true, ~0u, reached ? NX_OK : -99);
    }
    {   // refusal: an output that is also an input
        std::vector<u32> bits{5}, init{0}; std::vector<u32> col(4, 1), out(4, 0);
        const u32* kp[1] = {col.data()}; const u32* pp[1] = {col.data()}; u32* vp[1] = {col.data()};
        nx_access_stream s{kp, nullptr, pp, vp, nullptr, 2, 0, 0};
        nx_ctx ctx; u64 nk = 99;
        const int rc = nx_trace_prev_access(&ctx, &s, 1, 1, bits.data(), 1, init.data(), nullptr, &nk);
        const bool ok = rc == NX_ERR_ARG && nk == 99 && ctx.live == 0 && col[0] == 1;
        printf("%-58s rc %d %s  %s\n", "aliased output", rc, ok ? "OK" : "FAIL", ctx.err.c_str());
        ok ? n_ok++ : n_fail++;
    }
    printf("block cap %u\n%d cases OK\n%d failures\n", (unsigned)CP_MAX_BLOCKS, n_ok, n_fail);
    return n_fail != 0;
}
