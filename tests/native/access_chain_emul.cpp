// nx_trace_access_chain on the host: csrc/access_chain.hip (with csrc/access_history.cuh) compiled as plain C++ against tests/native/prev_emul/internal.h (256 lock-step
// threads per block as fibers, waves of 64 with ballot / shuffle, LDS as static storage), so the entry point with its kernels is checked
// word for word against a sequential walk over a map — under the address and undefined-behaviour sanitizers, which watch every LDS,
// histogram, placement, aggregate and summary index; every output has guard words behind it.  Built twice by the test: as it is, and with
// -DNX_COUNT_PASS_MAX_BLOCKS=2, where a block of the sort takes more tiles than the minimum.
#include "access_chain_emu.cpp"   // a copy of csrc/access_chain.hip next to the shim internal.h, access_history.cuh, trace_rows.h and count_pass.cuh (the test makes it)
#include <random>
#include <map>
#include <tuple>

static std::mt19937_64 rng(20261);
static int n_fail = 0, n_ok = 0;
static const u32 GUARD = 0xDEADBEEFu, TAIL = 4;

struct Stream {
    bool block = false;
    std::vector<std::vector<u32>> key;           // per key column: one word per position (column stream) or record (block stream)
    std::vector<u32> flag; bool has_flag = false;
    std::vector<std::vector<u32>> pay;           // per payload column: one word per element (bytes: values below 256); empty: NULL
    std::vector<u32> rule, delta; bool has_rule = true, has_delta = true;
    std::vector<char> prev_wanted; bool want_ord = true;
    std::vector<u32> row; u32 span = 0;          // block stream
    u32 log = 0, epoch = 0, linear = 0;
    size_t elems() const { return block ? row.size() * span : (size_t)1 << log; }
    size_t units() const { return block ? row.size() : (size_t)1 << log; }
};
static u32* dup_aligned(const std::vector<u32>& v, size_t misalign_words = 0) {
    u32* p = (u32*)aligned_alloc(256, ((v.size() + misalign_words) * 4 + 255 + 256) & ~(size_t)255);
    if (!v.empty()) memcpy(p + misalign_words, v.data(), v.size() * 4);
    return p + misalign_words;
}
static u32 model_row_of_pos(u32 pos, u32 log) {
    u32 d = 0; for (u32 b = 0; b < log; b++) d |= ((pos >> b) & 1u) << (log - 1 - b);
    const u32 n = 1u << log;
    return d < n / 2 ? 2 * d : 2 * (n - 1 - d) + 1;
}
struct Bad { u32 s, at, sub, kind; bool operator<(const Bad& o) const { return std::tie(s, at, sub, kind) < std::tie(o.s, o.at, o.sub, o.kind); } };
struct Want { std::vector<std::vector<std::vector<u32>>> prev; std::vector<std::vector<u32>> ord; std::vector<u32> skey, scount; std::vector<std::vector<u32>> slast; bool bad = false; Bad first{0, 0, 0, 0}; };
static Want model(const std::vector<Stream>& st, const std::vector<u32>& bits, u32 np, const std::vector<u32>& init) {
    struct Acc { u32 epoch, row, s, sub, unit; };
    std::vector<Acc> acc;
    Want w;
    auto bad = [&](Bad b) { if (!w.bad || b < w.first) w.first = b; w.bad = true; };
    u32 tb = 0; for (u32 b : bits) tb += b;
    for (u32 s = 0; s < st.size(); s++) {
        if (!st[s].block) { for (u32 pos = 0; pos < (1u << st[s].log); pos++) acc.push_back({st[s].epoch, st[s].linear ? pos : model_row_of_pos(pos, st[s].log), s, 0, pos}); continue; }
        for (u32 j = 0; j < st[s].row.size(); j++) {
            if (st[s].row[j] >> 31) bad({s, j, 0, 3}); else if (j && st[s].row[j - 1] >= st[s].row[j]) bad({s, j, 0, 2});
            for (u32 i = 0; i < st[s].span; i++) acc.push_back({st[s].epoch, st[s].row[j], s, i, j});
        }
    }
    std::sort(acc.begin(), acc.end(), [](const Acc& a, const Acc& b) { return std::tie(a.epoch, a.row, a.s, a.sub) < std::tie(b.epoch, b.row, b.s, b.sub); });
    w.prev.resize(st.size()); w.ord.resize(st.size());
    for (u32 s = 0; s < st.size(); s++) { w.prev[s].assign(np, std::vector<u32>(st[s].elems(), 0)); w.ord[s].assign(st[s].elems(), 0); }
    struct Last { std::vector<u32> state; u32 count; };
    std::map<u32, Last> last;
    for (const Acc& a : acc) {
        const Stream& S = st[a.s];
        if (S.has_flag && !S.flag[a.unit]) continue;
        u64 key = 0; u32 sh = 0; bool oor = false;
        for (size_t c = 0; c < bits.size(); c++) { const u32 x = S.key[c][a.unit]; if (bits[c] < 32 && (x >> bits[c])) oor = true; key |= (u64)(u32)(x << sh); sh += bits[c]; }
        if (oor) { bad({a.s, a.unit, 0, 0}); continue; }
        key += a.sub;
        if (key >> tb) { bad({a.s, a.unit, a.sub, 1}); continue; }
        const size_t el = S.block ? (size_t)a.unit * S.span + a.sub : a.unit;
        auto it = last.find((u32)key);
        if (it == last.end()) it = last.insert({(u32)key, Last{init, 0}}).first;
        Last& l = it->second;
        for (u32 c = 0; c < np; c++) {
            w.prev[a.s][c][el] = l.state[c];
            const u32 ru = S.has_rule ? S.rule[c] : 0;
            if (ru & 1) l.state[c] += S.has_delta ? S.delta[c] : 1u; else l.state[c] = S.pay[c].empty() ? 0 : S.pay[c][el];
        }
        w.ord[a.s][el] = l.count++;
    }
    w.slast.resize(np);
    for (auto& kv : last) { w.skey.push_back(kv.first); w.scount.push_back(kv.second.count); for (u32 c = 0; c < np; c++) w.slast[c].push_back(kv.second.state[c]); }
    return w;
}

static void run_case(const char* name, std::vector<Stream>& st, const std::vector<u32>& bits, u32 np, const std::vector<u32>& init, bool with_summary, u32 cap, int expect_rc,
                     size_t misalign = 0) {
    const Want w = model(st, bits, np, init);
    nx_ctx ctx;
    const u32 k = bits.size(), ns = st.size();
    std::vector<std::vector<const u32*>> kp(ns), pp(ns); std::vector<std::vector<u32*>> vp(ns); std::vector<u32*> op(ns, nullptr);
    std::vector<nx_chain_stream> cs(ns);
    u64 elems = 0;
    for (u32 s = 0; s < ns; s++) {
        const size_t n = st[s].elems();
        elems += n;
        for (u32 c = 0; c < k; c++) kp[s].push_back(dup_aligned(st[s].key[c], misalign));
        for (u32 c = 0; c < np; c++) {
            if (st[s].pay[c].empty()) { pp[s].push_back(nullptr); continue; }
            if (st[s].has_rule && (st[s].rule[c] & 2)) {          // bytes: packed, 4-byte aligned at every placement
                std::vector<u32> packed(n / 4, 0);
                for (size_t e = 0; e < n; e++) packed[e / 4] |= st[s].pay[c][e] << (8 * (e % 4));
                pp[s].push_back(dup_aligned(packed, misalign));
            } else pp[s].push_back(dup_aligned(st[s].pay[c], misalign));
        }
        for (u32 c = 0; c < np && !st[s].prev_wanted.empty(); c++) vp[s].push_back(st[s].prev_wanted[c] ? dup_aligned(std::vector<u32>(n + TAIL, GUARD), misalign) : nullptr);
        if (st[s].want_ord) op[s] = dup_aligned(std::vector<u32>(n + TAIL, GUARD), misalign);
        memset(&cs[s], 0, sizeof cs[s]);
        cs[s].d_key = kp[s].data(); cs[s].d_flag = st[s].has_flag ? dup_aligned(st[s].flag, misalign) : nullptr; cs[s].d_payload = pp[s].data();
        cs[s].d_row = st[s].block ? dup_aligned(st[s].row, misalign) : nullptr;
        cs[s].rule = st[s].has_rule ? st[s].rule.data() : nullptr; cs[s].delta = st[s].has_delta ? st[s].delta.data() : nullptr;
        cs[s].d_prev = st[s].prev_wanted.empty() ? nullptr : vp[s].data(); cs[s].d_ordinal = op[s];
        cs[s].log_size = st[s].log; cs[s].epoch = st[s].epoch; cs[s].linear = st[s].linear; cs[s].n_records = st[s].block ? (u32)st[s].row.size() : 0; cs[s].span = st[s].span;
    }
    const u32 nk = (u32)w.skey.size(), real_cap = cap == ~0u ? nk : cap;
    nx_access_summary sum; std::vector<u32*> lastp;
    sum.cap = real_cap; sum.d_key = dup_aligned(std::vector<u32>(real_cap + TAIL, GUARD)); sum.d_count = dup_aligned(std::vector<u32>(real_cap + TAIL, GUARD));
    for (u32 c = 0; c < np; c++) lastp.push_back(dup_aligned(std::vector<u32>(real_cap + TAIL, GUARD)));
    sum.d_last = lastp.data();
    u64 got_keys = 99;
    const int rc = nx_trace_access_chain(&ctx, cs.data(), ns, k, bits.data(), np, init.data(), with_summary ? &sum : nullptr, &got_keys);
    bool ok = rc == expect_rc && ctx.live == 0 && ctx.live_bytes == 0;
    std::string why;
    if (ctx.peak_bytes > 18 * elems + 1024 * (u64)ns + 65536) { ok = false; why = "peak of " + std::to_string(ctx.peak_bytes) + " bytes above the documented bound"; }
    if (rc == NX_OK) {
        for (u32 s = 0; s < ns && ok; s++) {
            const size_t n = st[s].elems();
            for (size_t p = 0; p < n + TAIL && ok; p++) {
                if (op[s] && op[s][p] != (p < n ? w.ord[s][p] : GUARD)) { ok = false; why = "ordinal of stream " + std::to_string(s) + " element " + std::to_string(p) + ": " + std::to_string(op[s][p]); }
                for (u32 c = 0; c < np && ok && !st[s].prev_wanted.empty(); c++)
                    if (vp[s][c] && vp[s][c][p] != (p < n ? w.prev[s][c][p] : GUARD)) { ok = false; why = "prev " + std::to_string(c) + " of stream " + std::to_string(s) + " element " + std::to_string(p) + ": " + std::to_string(vp[s][c][p]) + " want " + std::to_string(p < n ? w.prev[s][c][p] : GUARD); }
            }
        }
        if (got_keys != nk) { ok = false; why = "n_keys " + std::to_string(got_keys) + " want " + std::to_string(nk); }
        for (u32 i = 0; i < real_cap + TAIL && ok; i++) {
            const bool in = with_summary && i < std::min(real_cap, nk);
            if (sum.d_key[i] != (in ? w.skey[i] : GUARD) || sum.d_count[i] != (in ? w.scount[i] : GUARD)) { ok = false; why = "summary entry " + std::to_string(i); }
            for (u32 c = 0; c < np && ok; c++) if (lastp[c][i] != (in ? w.slast[c][i] : GUARD)) { ok = false; why = "summary last " + std::to_string(c) + " entry " + std::to_string(i) + ": " + std::to_string(lastp[c][i]); }
        }
    } else if (rc == NX_ERR_PROTOCOL) {
        std::string at = "stream " + std::to_string(w.first.s) + (st[w.first.s].block ? " record " : " row position ") + std::to_string(w.first.at);
        at += w.first.kind == 1 ? " sub-access " + std::to_string(w.first.sub) + ":" : ":";
        const char* words[4] = {"key entry", "key bits", "not above its predecessor's", "not below 2^31"};
        if (!w.bad || ctx.err.find(at) == std::string::npos || ctx.err.find(words[w.first.kind]) == std::string::npos) { ok = false; why = "message does not name " + at + " " + words[w.first.kind]; }
        if (got_keys != 99) { ok = false; why = "n_keys written on an error"; }
    }
    if (rc == NX_OK && w.bad) { ok = false; why = "the model refuses this input"; }
    printf("%-66s rc %d (want %d) keys %llu %s  %s %s\n", name, rc, expect_rc, (unsigned long long)got_keys, ok ? "OK" : "FAIL", why.c_str(), rc ? ctx.err.c_str() : "");
    ok ? n_ok++ : n_fail++;
}

// rule_mode 0: all GIVEN; 1: random GIVEN / ADD per column; 2: all ADD.  Keys: base + a few values, so that runs are long.
static void fill_payload(Stream& S, u32 np, int rule_mode, bool bytes_ok) {
    const size_t n = S.elems();
    S.pay.assign(np, {}); S.rule.assign(np, 0); S.delta.assign(np, 1);
    for (u32 c = 0; c < np; c++) {
        const bool add = rule_mode == 2 || (rule_mode == 1 && (rng() & 1));
        S.rule[c] = add ? NX_CHAIN_ADD : NX_CHAIN_GIVEN;
        const u32 deltas[5] = {1u, 0u, 0xFFFFFFFFu, 7u, (u32)rng()};
        S.delta[c] = deltas[rng() % 5];
        if (add) continue;
        if (rng() % 6 == 0) continue;                              // a NULL payload column
        const bool bytes = bytes_ok && S.block && S.span % 4 == 0 && (rng() & 1);
        if (bytes) S.rule[c] |= NX_CHAIN_BYTES;
        S.pay[c].resize(n); for (auto& x : S.pay[c]) x = bytes ? (u32)(rng() & 255) : (u32)rng();
    }
    S.prev_wanted.assign(np, 1); for (u32 c = 0; c < np; c++) if (rng() % 7 == 0) S.prev_wanted[c] = 0;
    S.want_ord = rng() % 5 != 0;
}
static void set_keys(Stream& S, const std::vector<u32>& bits, u32 key_space, bool flags) {
    const size_t n = S.units();
    u32 tb = 0; for (u32 b : bits) tb += b;
    S.key.assign(bits.size(), std::vector<u32>(n));
    const u64 top = ((u64)1 << tb) - (S.block ? S.span : 1);       // the last sub-access stays inside the key bits
    for (size_t p = 0; p < n; p++) {
        const u64 key = std::min<u64>(top, (rng() % 4 == 0 ? (top > key_space ? top - rng() % key_space : 0) : rng() % key_space));
        u32 sh = 0;
        for (size_t c = 0; c < bits.size(); c++) { S.key[c][p] = (u32)((key >> sh) & (((u64)1 << bits[c]) - 1)); sh += bits[c]; }
    }
    S.has_flag = flags; S.flag.resize(n); for (auto& x : S.flag) x = (rng() % 4) ? (u32)(1 + rng() % 5) : 0;
}
static Stream column_stream(const std::vector<u32>& bits, u32 log, u32 np, int rule_mode, bool flags, u32 key_space, u32 epoch = 0, u32 linear = 0) {
    Stream S; S.log = log; S.epoch = epoch; S.linear = linear;
    set_keys(S, bits, key_space, flags); fill_payload(S, np, rule_mode, false);
    return S;
}
// rows: n_records distinct rows below max_row, ascending
static Stream block_stream(const std::vector<u32>& bits, u32 n_records, u32 span, u32 max_row, u32 np, int rule_mode, bool flags, u32 key_space, u32 epoch = 0) {
    Stream S; S.block = true; S.span = span; S.epoch = epoch;
    std::vector<u32> all(max_row); for (u32 i = 0; i < max_row; i++) all[i] = i;
    std::shuffle(all.begin(), all.end(), rng); all.resize(n_records); std::sort(all.begin(), all.end());
    S.row = all;
    set_keys(S, bits, key_space, flags); fill_payload(S, np, rule_mode, true);
    return S;
}
// one linear stream of 2^log rows whose first `n` rows access key 5 by ADD, and a second one of 2 rows that may put one GIVEN at `given_row`
static void one_key_chain(u32 n, int given_at, u32 delta, u32 init0) {
    const std::vector<u32> bits{13};
    u32 log = 1; while ((1u << log) < n) log++;
    std::vector<Stream> st(2);
    Stream& A = st[0]; A.log = log; A.linear = 1; A.key.assign(1, std::vector<u32>((size_t)1 << log, 5)); A.has_flag = true; A.flag.assign((size_t)1 << log, 0);
    for (u32 i = 0; i < n; i++) A.flag[i] = 1;
    A.pay.assign(2, {}); A.pay[1].resize((size_t)1 << log); for (auto& x : A.pay[1]) x = (u32)rng();
    A.rule = {NX_CHAIN_ADD, NX_CHAIN_GIVEN}; A.delta = {delta, 0}; A.prev_wanted = {1, 1};
    // the second stream: one record of span 1 at the row of the GIVEN (a block stream: any row can be named), later in `streams`, so it follows A's access of that row
    Stream& G = st[1]; G.block = true; G.span = 1; G.row = {given_at < 0 ? 0u : (u32)given_at}; G.key.assign(1, std::vector<u32>(1, 5)); G.has_flag = true; G.flag = {given_at < 0 ? 0u : 1u};
    G.pay.assign(2, {}); G.pay[0] = {0x80000001u}; G.pay[1] = {77}; G.rule = {NX_CHAIN_GIVEN, NX_CHAIN_GIVEN}; G.has_delta = false; G.prev_wanted = {1, 1};
    char nm[96]; snprintf(nm, 96, "one key %u times by ADD %u, GIVEN at %d, init %u", n, delta, given_at, init0);
    run_case(nm, st, bits, 2, {init0, 3}, true, ~0u, NX_OK);
}

int main() {
    const std::vector<std::vector<u32>> keyings = {{5}, {8, 5}, {8, 8, 8, 8}, {31}};
    // compatibility shapes: column streams, every rule GIVEN
    for (auto& bits : keyings)
        for (u32 log : {1u, 6u, 11u}) {
            std::vector<Stream> st; for (u32 s = 0; s < 3; s++) st.push_back(column_stream(bits, log, 3, 0, s & 1, 40));
            st[1].has_rule = false; st[2].has_delta = false;
            char nm[96]; snprintf(nm, 96, "GIVEN only, %zu key cols, 3 streams of 2^%u", bits.size(), log);
            run_case(nm, st, bits, 3, {1, 2, 3}, true, ~0u, NX_OK, log == 6 ? 1 : 0);
        }
    // chains across every boundary of the scan
    for (u32 n : {1u, 2u, 3u, 4u, 5u, 1023u, 1024u, 1025u, 2049u, 3000u}) {
        one_key_chain(n, -1, 1, 0);
        one_key_chain(n, 0, 0xFFFFFFFFu, 9); one_key_chain(n, (int)(n / 2), 0, 1000); one_key_chain(n, (int)(n - 1), 3, P - 1);
    }
    // mixed: column and block streams, random rules per stream and column, epochs, flags, overlapping buffers, bytes
    int variant = 0;
    for (auto& bits : keyings)
        for (u32 span : {1u, 4u, 200u, 256u})
            for (u32 n_rec : {0u, 1u, 2u, 5u, 40u}) {
                u32 tb = 0; for (u32 b : bits) tb += b;
                if ((1u << std::min(tb, 30u)) <= span) continue;
                if ((variant++ % 3) && n_rec == 40 && span >= 200) continue;   // the large ones a third of the time
                const u32 np = 1 + variant % 4, logs[] = {2, 6, 10}, log = logs[variant % 3], space = std::min<u32>(400, (1u << std::min(tb, 30u)) - span);
                std::vector<Stream> st;
                st.push_back(column_stream(bits, 4, np, 0, false, space, 0, 1)); st[0].prev_wanted.clear();       // an image
                st.push_back(column_stream(bits, log, np, 1, variant & 1, space, 1));
                st.push_back(block_stream(bits, n_rec, span, std::max((1u << log) + 3, n_rec + 5), np, 1, variant & 2, space, 1));
                st.push_back(column_stream(bits, log, np, 1, true, space, 1));
                const u32 n_more = variant % 5 == 0 ? 7 : variant % 2;
                for (u32 b = 0; b < n_more; b++) st.push_back(block_stream(bits, 1 + (b + n_rec) % 4, b % 2 ? span : 4, 1u << log, np, b % 3, b & 1, space, 1));
                if (n_rec) { st[2].row.front() = 0; if (n_rec > 1) st[2].row.back() = (1u << log) - 1 > st[2].row[n_rec - 2] ? (1u << log) - 1 : st[2].row.back(); }
                st.push_back(column_stream(bits, 3, np, 2, false, space, 9));
                std::vector<u32> init(np); for (auto& x : init) x = (u32)(rng() % P);
                char nm[112]; snprintf(nm, 112, "mixed: %zu key cols, span %u, %u records, 2^%u rows, %u payload, %u more block streams", bits.size(), span, n_rec, log, np, n_more);
                run_case(nm, st, bits, np, init, variant % 4 != 0, variant % 7 == 0 ? 3 : ~0u, NX_OK, variant % 4);
            }
    {   // records on consecutive rows hashing one buffer, and a second buffer overlapping it by 8 keys
        const std::vector<u32> bits{16};
        std::vector<Stream> st;
        st.push_back(column_stream(bits, 6, 2, 0, false, 300, 1)); st[0].rule = {0, 0};
        Stream B = block_stream(bits, 5, 200, 64, 2, 0, false, 300, 1);
        B.row = {3, 4, 5, 20, 63}; B.key[0] = {10, 10, 10, 202, 202}; B.rule = {NX_CHAIN_ADD, NX_CHAIN_GIVEN | NX_CHAIN_BYTES}; B.pay[0].clear(); B.pay[1].resize(1000); for (auto& x : B.pay[1]) x = (u32)(rng() & 255);
        B.prev_wanted = {1, 1}; B.want_ord = true;
        st.push_back(B);
        run_case("absorb loop: three records in a row, overlap of 8", st, bits, 2, {0, 0}, true, ~0u, NX_OK);
    }
    {   // only block streams without records: no element at all
        const std::vector<u32> bits{8};
        std::vector<Stream> st; st.push_back(block_stream(bits, 0, 4, 8, 1, 2, false, 10));
        run_case("no element", st, bits, 1, {5}, true, ~0u, NX_OK);
    }
    {   // 2^11 + 2 * 4 elements: with a block cap of 2 (the second build) a sort block takes more tiles than the minimum in each pass
        const std::vector<u32> bits{8, 5}, init{P - 3};
        std::vector<Stream> st;
        st.push_back(column_stream(bits, 11, 1, 2, true, 300, 0, 1));
        st.push_back(block_stream(bits, 2, 4, 2048, 1, 1, false, 300));
        const CountPlan plan = count_plan(((u64)1 << 11) + 8);
        const bool reached = CP_MAX_BLOCKS != 2 || (plan.tiles > CP_MIN_TILES && plan.blocks == 2);
        run_case(reached ? "  2^11 rows and two records of 4" : "  2^11 rows and two records of 4: PLAN NOT REACHED", st, bits, 1, init, true, ~0u, reached ? NX_OK : -99);
    }
    {   // refused by the device: named as (stream, position or record, sub-access), smallest first
        const std::vector<u32> bits{8, 5}, init{0, 0};
        auto fresh = [&]() {
            std::vector<Stream> st;
            st.push_back(column_stream(bits, 6, 2, 1, true, 300));
            st.push_back(block_stream(bits, 5, 8, 64, 2, 1, true, 300));
            st.push_back(block_stream(bits, 3, 4, 64, 2, 1, false, 300));
            return st;
        };
        { auto st = fresh(); st[1].key[0][3] = 256; st[1].flag[3] = 0; run_case("  entry out of its bits on a record that does not access", st, bits, 2, init, true, ~0u, NX_OK); }
        { auto st = fresh(); st[1].key[0][3] = 256; st[1].flag[3] = 1; st[2].key[1][0] = 32; run_case("  entry out of its bits on a record", st, bits, 2, init, true, ~0u, NX_ERR_PROTOCOL); }
        { auto st = fresh(); st[1].key[0][2] = 250; st[1].key[1][2] = 31; st[1].flag[2] = 1; run_case("  sub-access past the key bits", st, bits, 2, init, true, ~0u, NX_ERR_PROTOCOL); }
        { auto st = fresh(); st[2].row = {7, 7, 9}; run_case("  equal rows", st, bits, 2, init, true, ~0u, NX_ERR_PROTOCOL); }
        { auto st = fresh(); st[1].row = {1, 9, 5, 4, 30}; st[1].flag[2] = 0; run_case("  descending rows, on a record that does not access", st, bits, 2, init, false, ~0u, NX_ERR_PROTOCOL); }
        { auto st = fresh(); st[2].row = {1, 2, 0x80000000u}; run_case("  a row of 2^31", st, bits, 2, init, true, ~0u, NX_ERR_PROTOCOL); }
        { auto st = fresh(); st[0].key[1][40] = 32; st[0].flag[40] = 1; st[1].row = {5, 4, 3, 2, 1}; run_case("  a column stream's row before a block stream's record", st, bits, 2, init, true, ~0u, NX_ERR_PROTOCOL); }
    }
    {   // keys up to 2^32 - 1: the last sub-access on the last key, and one past it
        const std::vector<u32> bits{16, 16}, init{4};
        std::vector<Stream> st; st.push_back(block_stream(bits, 2, 4, 9, 1, 2, false, 10));
        st[0].key[0] = {0xFFFC, 0xFFF8}; st[0].key[1] = {0xFFFF, 0xFFFF};
        run_case("  the last key of 32 bits", st, bits, 1, init, true, ~0u, NX_OK);
        st[0].key[0][1] = 0xFFFD;
        run_case("  one past the last key of 32 bits", st, bits, 1, init, true, ~0u, NX_ERR_PROTOCOL);
    }
    {   // refusal: an output that is also an input
        std::vector<u32> bits{5}, init{0}; std::vector<u32> col(4, 1);
        const u32* kp[1] = {col.data()}; const u32* pp[1] = {col.data()}; u32* vp[1] = {col.data()};
        nx_chain_stream s; memset(&s, 0, sizeof s); s.d_key = kp; s.d_payload = pp; s.d_prev = vp; s.log_size = 2;
        nx_ctx ctx; u64 nk = 99;
        const int rc = nx_trace_access_chain(&ctx, &s, 1, 1, bits.data(), 1, init.data(), nullptr, &nk);
        const bool ok = rc == NX_ERR_ARG && nk == 99 && ctx.live == 0 && col[0] == 1;
        printf("%-66s rc %d %s  %s\n", "aliased output", rc, ok ? "OK" : "FAIL", ctx.err.c_str());
        ok ? n_ok++ : n_fail++;
    }
    printf("block cap %u\n%d cases OK\n%d failures\n", (unsigned)CP_MAX_BLOCKS, n_ok, n_fail);
    return n_fail != 0;
}
