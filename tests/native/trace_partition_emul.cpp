// nx_trace_partition_create / _fill on the host: csrc/trace_partition.hip compiled as plain C++ against the lock-step shim
// (tests/native/prev_emul/internal.h with tests/native/part_emul/shim.h on top), so the entry points with their kernels are compared
// word for word with a sequential filter-and-enumerate walk over the step table — under the address and undefined-behaviour
// sanitizers, which watch every LDS, histogram, order and descriptor index.  Built twice by the test: as it is, and with
// -DNX_COUNT_PASS_MAX_BLOCKS=2, where a block of the counting pass takes more tiles than the minimum.
#include "shim.h"
#include "trace_partition_emu.cpp"   // a copy of csrc/trace_partition.hip next to the shim, trace_rows.h and count_pass.cuh (the test makes it)
#include <random>

static std::mt19937_64 rng(7102);
static int n_fail = 0, n_ok = 0;
static const u32 GUARD = 0xDEADBEEFu, N_GUARD = 4;

static void report(bool ok, const std::string& name) {
    if (ok) { n_ok++; printf(" OK   %s\n", name.c_str()); } else { n_fail++; printf(" FAIL %s\n", name.c_str()); }
}
// the model's own row of a storage position, from the definition: position = bitrev(index in the circle domain), the domain holds
// the even coset rows in its first half and the odd ones, backwards, in its second
static u32 model_row_of_pos(u32 pos, u32 log) {
    u32 d = 0; for (u32 b = 0; b < log; b++) d |= ((pos >> b) & 1u) << (log - 1 - b);
    const u32 n = 1u << log;
    return d < n / 2 ? 2 * d : 2 * (n - 1 - d) + 1;
}
static u32 model_limb(u32 w, nx_part_limb l) { const u32 v = (u32)(((u64)w >> l.shift) & (((u64)1 << l.bits) - 1)); return v == P ? 0 : v; }
static u32 model_log(u64 count, u32 min_log) { u32 l = 0; while (((u64)1 << l) < count) l++; return std::max(l, min_log); }

// an output of exactly n words + guard words, filled with a pattern no result has
struct Out {
    u32* p; size_t n;
    explicit Out(size_t n_) : p((u32*)malloc((n_ + N_GUARD) * 4)), n(n_) { for (size_t i = 0; i < n + N_GUARD; i++) p[i] = GUARD; }
    bool guards() const { for (u32 i = 0; i < N_GUARD; i++) if (p[n + i] != GUARD) return false; return true; }
    bool untouched() const { for (size_t i = 0; i < n + N_GUARD; i++) if (p[i] != GUARD) return false; return true; }
};

struct Dest { u32 cls, log; std::vector<nx_part_limb> limbs; bool pad, step; };
static const std::vector<nx_part_limb> SPECS = {{0, 0, 8}, {0, 8, 8}, {0, 16, 16}, {1, 2, 6}, {1, 0, 1}, {1, 31, 1}, {2, 0, 31}, {2, 1, 31},
                                                {3, 0, 8}, {3, 8, 8}, {3, 16, 8}, {3, 24, 8}, {3, 0, 16}, {3, 16, 16}};   // one source read by six specs

enum Dist { UNIFORM, ONE_CLASS, ALL_BUT_ONE, SORTED, ALTERNATE, RUN64, RUN65, WITH_NONE, ALL_NONE, SPARSE };
static const char* DIST_NAME[] = {"uniform", "one-class", "all-but-one", "sorted", "alternate", "run64", "run65", "with-none", "all-none", "sparse"};
static std::vector<u32> classes(u32 n, u32 k, Dist d) {
    std::vector<u32> c(n);
    for (u32 j = 0; j < n; j++) {
        switch (d) {
        case UNIFORM: c[j] = (u32)(rng() % k); break;
        case ONE_CLASS: c[j] = k - 1; break;
        case ALL_BUT_ONE: c[j] = j == n / 2 ? 0 : k - 1; break;
        case SORTED: c[j] = (u32)((u64)j * k / std::max(1u, n)); break;
        case ALTERNATE: c[j] = (j & 1) ? k - 1 : 0; break;
        case RUN64: c[j] = (j / 64) % k; break;
        case RUN65: c[j] = (j / 65) % k; break;
        case WITH_NONE: c[j] = rng() % 3 == 0 ? NX_PART_NONE : (u32)(rng() % k); break;
        case ALL_NONE: c[j] = NX_PART_NONE; break;
        case SPARSE: c[j] = (u32)(rng() % 2 ? 0 : (k - 1) / 2); break;      // classes that never occur
        }
    }
    return c;
}

static bool run_case(u32 n, u32 k, Dist dist, u32 extra_log, bool opt_cols, const std::string& name) {
    nx_ctx ctx;
    const std::vector<u32> cls = classes(n, k, dist);
    const u32 n_src = 4;
    std::vector<std::vector<u32>> src(n_src, std::vector<u32>(n));
    for (auto& col : src) for (u32& w : col) w = (u32)rng();
    for (u32 j = 0; j < n; j += 3) src[2][j] = P;                 // (0, 31) of p is written as 0
    u32* d_cls = (u32*)malloc(std::max<size_t>(1, n) * 4); if (n) memcpy(d_cls, cls.data(), (size_t)n * 4);
    std::vector<u32*> d_src(n_src);
    for (u32 s = 0; s < n_src; s++) { d_src[s] = (u32*)malloc(std::max<size_t>(1, n) * 4); if (n) memcpy(d_src[s], src[s].data(), (size_t)n * 4); }
    // the walk: the steps of every class in execution order
    std::vector<std::vector<u32>> rows(k);
    for (u32 j = 0; j < n; j++) if (cls[j] < k) rows[cls[j]].push_back(j);
    std::vector<u32> all(n); for (u32 j = 0; j < n; j++) all[j] = j;

    std::vector<u32> counts(k, 77);
    nx_partition* part = nullptr;
    bool ok = true;
    int rc = nx_trace_partition_create(&ctx, n ? d_cls : nullptr, n, k, counts.data(), &part);
    if (rc != NX_OK || !part) { printf("   create: rc %d %s\n", rc, ctx.err.c_str()); report(false, name); return false; }
    for (u32 c = 0; c < k; c++) if (counts[c] != rows[c].size()) { printf("   count of class %u: %u, %zu expected\n", c, counts[c], rows[c].size()); ok = false; }
    if (ctx.live != (n ? 1u : 0u) || ctx.live_bytes != (size_t)n * 4) { printf("   live after create: %zu blocks %zu bytes\n", ctx.live, ctx.live_bytes); ok = false; }
    if (ctx.peak_bytes > (size_t)n * 4 + 4 * (size_t)k * CP_MAX_BLOCKS + 1280 + 256) { printf("   peak %zu bytes above the header's bound\n", ctx.peak_bytes); ok = false; }

    // every class and NX_PART_ALL; class 0 twice (two destinations of one class in one call)
    std::vector<Dest> dests;
    for (u32 c = 0; c <= k + 1; c++) {
        const u32 cl = c < k ? c : c == k ? NX_PART_ALL : 0;
        const size_t cnt = cl == NX_PART_ALL ? n : rows[cl].size();
        Dest d; d.cls = cl; d.log = model_log(cnt, (c & 1) ? 4 : 1) + ((c % 3 == 2) ? extra_log : 0);
        const size_t take = k > 8 && c < k ? 1 + c % 5 : SPECS.size();        // many classes: a few specs each keeps the run short
        for (size_t i = 0; i < take; i++) d.limbs.push_back(SPECS[(i + (k > 8 ? c : 0)) % SPECS.size()]);
        d.pad = opt_cols || (c & 1); d.step = opt_cols || (c & 2);
        if (nx_trace_partition_log_size(cnt, (c & 1) ? 4 : 1) != model_log(cnt, (c & 1) ? 4 : 1)) { printf("   log_size helper at %zu\n", cnt); ok = false; }
        dests.push_back(d);
    }
    std::vector<nx_part_dest> h(dests.size());
    std::vector<std::vector<Out>> outs(dests.size());
    std::vector<std::vector<u32*>> ptrs(dests.size());
    std::vector<Out> pads, steps;
    for (size_t i = 0; i < dests.size(); i++) {
        const size_t rows_n = (size_t)1 << dests[i].log;
        for (size_t c = 0; c < dests[i].limbs.size(); c++) { outs[i].emplace_back(rows_n); }
        for (auto& o : outs[i]) ptrs[i].push_back(o.p);
        pads.emplace_back(rows_n); steps.emplace_back(rows_n);
        h[i].cls = dests[i].cls; h[i].log_size = dests[i].log; h[i].n_cols = (u32)dests[i].limbs.size(); h[i].d_cols = ptrs[i].data(); h[i].limbs = dests[i].limbs.data();
        h[i].d_is_pad = dests[i].pad ? pads[i].p : nullptr; h[i].d_step = dests[i].step ? steps[i].p : nullptr;
    }
    rc = nx_trace_partition_fill(&ctx, part, d_src.data(), n_src, h.data(), (u32)h.size());
    if (rc != NX_OK) { printf("   fill: rc %d %s\n", rc, ctx.err.c_str()); ok = false; }
    if (ctx.live != (n ? 1u : 0u)) { printf("   the fill allocated device memory\n"); ok = false; }
    for (size_t i = 0; i < dests.size() && rc == NX_OK; i++) {
        const std::vector<u32>& R = dests[i].cls == NX_PART_ALL ? all : rows[dests[i].cls];
        const u32 log = dests[i].log;
        for (u32 pos = 0; pos < (1u << log); pos++) {
            const u32 r = model_row_of_pos(pos, log); const bool real = r < R.size();
            for (size_t c = 0; c < dests[i].limbs.size(); c++) {
                const u32 want = real ? model_limb(src[dests[i].limbs[c].src][R[r]], dests[i].limbs[c]) : 0;
                if (outs[i][c].p[pos] != want) { if (ok) printf("   dest %zu col %zu pos %u: %u, %u expected\n", i, c, pos, outs[i][c].p[pos], want); ok = false; }
            }
            if (dests[i].pad && pads[i].p[pos] != (real ? 0u : 1u)) { if (ok) printf("   dest %zu is_pad pos %u\n", i, pos); ok = false; }
            if (dests[i].step && steps[i].p[pos] != (real ? R[r] : 0u)) { if (ok) printf("   dest %zu step pos %u\n", i, pos); ok = false; }
        }
        for (auto& o : outs[i]) if (!o.guards()) { printf("   dest %zu: a guard word was written\n", i); ok = false; }
        if (!(dests[i].pad ? pads[i].guards() : pads[i].untouched()) || !(dests[i].step ? steps[i].guards() : steps[i].untouched())) { printf("   dest %zu: optional output\n", i); ok = false; }
    }
    nx_trace_partition_destroy(part);
    if (ctx.live != 0 || ctx.live_bytes != 0) { printf("   live after destroy: %zu blocks\n", ctx.live); ok = false; }
    staged_release();
    for (auto& v : outs) for (auto& o : v) free(o.p);
    for (auto& o : pads) free(o.p);
    for (auto& o : steps) free(o.p);
    for (u32* p : d_src) free(p);
    free(d_cls);
    report(ok, name);
    return ok;
}

// a class word outside the classes: the smallest such step is named, nothing is kept, the context partitions a good table afterwards
static void refused_class(u32 bad_word) {
    nx_ctx ctx;
    const u32 n = 1500, k = 40;
    std::vector<u32> cls = classes(n, k, WITH_NONE);
    cls[1234] = bad_word; cls[417] = bad_word; cls[418] = k + 7;
    std::vector<u32> counts(k, 77);
    nx_partition* part = (nx_partition*)(uintptr_t)16;
    const int rc = nx_trace_partition_create(&ctx, cls.data(), n, k, counts.data(), &part);
    const std::string want = "nx_trace_partition_create: step 417: class " + std::to_string(bad_word) + ", 40 classes";
    bool ok = rc == NX_ERR_PROTOCOL && ctx.err == want && part == nullptr && ctx.live == 0 && ctx.live_bytes == 0;
    if (!ok) printf("   rc %d '%s' live %zu\n", rc, ctx.err.c_str(), ctx.live);
    cls[1234] = 0; cls[417] = 1; cls[418] = 2;
    ok = ok && nx_trace_partition_create(&ctx, cls.data(), n, k, counts.data(), &part) == NX_OK && part;
    if (part) nx_trace_partition_destroy(part);
    report(ok && ctx.live == 0, "refused class word " + std::to_string(bad_word));
}

// every NX_ERR_ARG of the fill: nothing is launched, the outputs keep their pattern
static void refused_fill() {
    nx_ctx ctx, other;
    const u32 n = 300, k = 3;
    std::vector<u32> cls = classes(n, k, UNIFORM), s0(n, 5), s1(n, 6), counts(k);
    nx_partition* part = nullptr;
    if (nx_trace_partition_create(&ctx, cls.data(), n, k, counts.data(), &part) != NX_OK) { report(false, "refusals: create"); return; }
    auto attempt = [&](const char* text, const std::function<void(nx_part_dest*, std::vector<nx_part_limb>&, std::vector<u32*>&, const u32**, u32*)>& breakit, nx_ctx* use = nullptr,
                       bool null_part = false) {
        Out a(512), b(512), pad(512), step(512), a2(512);
        std::vector<nx_part_limb> limbs = {{0, 0, 8}, {1, 8, 8}}, limbs2 = {{1, 0, 31}};
        std::vector<u32*> cols = {a.p, b.p}, cols2 = {a2.p};
        nx_part_dest d[2] = {{0, 9, 2, nullptr, nullptr, pad.p, step.p}, {NX_PART_ALL, 9, 1, nullptr, nullptr, nullptr, nullptr}};
        const u32* srcs[2] = {s0.data(), s1.data()};
        u32 n_src = 2;
        breakit(d, limbs, cols, srcs, &n_src);
        d[0].d_cols = d[0].d_cols == (u32* const*)(uintptr_t)1 ? nullptr : cols.data(); d[0].limbs = d[0].limbs == (const nx_part_limb*)(uintptr_t)1 ? nullptr : limbs.data();
        d[1].d_cols = cols2.data(); d[1].limbs = limbs2.data();
        nx_ctx* c = use ? use : &ctx;
        c->err.clear();
        const int rc = nx_trace_partition_fill(c, null_part ? nullptr : part, srcs, n_src, d, 2);
        const bool ok = rc == NX_ERR_ARG && c->err.rfind("nx_trace_partition_fill: ", 0) == 0 && c->err.find(text) != std::string::npos && a.untouched() && b.untouched() &&
                        pad.untouched() && step.untouched() && a2.untouched();
        if (!ok) printf("   rc %d '%s'\n", rc, c->err.c_str());
        report(ok, std::string("refusal: ") + text);
        free(a.p); free(b.p); free(pad.p); free(step.p); free(a2.p);
    };
    typedef nx_part_dest* D; typedef std::vector<nx_part_limb>& L; typedef std::vector<u32*>& Cv;
    attempt("NULL partition", [](D, L, Cv, const u32**, u32*) {}, nullptr, true);
    attempt("another context", [](D, L, Cv, const u32**, u32*) {}, &other);
    attempt("destination 0: class 3, 3 classes", [](D d, L, Cv, const u32**, u32*) { d[0].cls = 3; });
    attempt("destination 0: class 4294967294", [](D d, L, Cv, const u32**, u32*) { d[0].cls = 0xFFFFFFFEu; });
    attempt("destination 0: log_size of 0", [](D d, L, Cv, const u32**, u32*) { d[0].log_size = 0; });
    attempt("destination 0: log_size of 31", [](D d, L, Cv, const u32**, u32*) { d[0].log_size = 31; });
    attempt("destination 1: log_size of 8, its 300 steps do not fit", [](D d, L, Cv, const u32**, u32*) { d[1].log_size = 8; });
    attempt("destination 0 column 1: src of 2, 2 source columns", [](D, L l, Cv, const u32**, u32*) { l[1].src = 2; });
    attempt("destination 0 column 0: shift 0 bits 0", [](D, L l, Cv, const u32**, u32*) { l[0].bits = 0; });
    attempt("destination 0 column 0: shift 0 bits 32", [](D, L l, Cv, const u32**, u32*) { l[0].bits = 32; });
    attempt("destination 0 column 1: shift 25 bits 8", [](D, L l, Cv, const u32**, u32*) { l[1].shift = 25; });
    attempt("destination 0 column 1: NULL output column", [](D, L, Cv c, const u32**, u32*) { c[1] = nullptr; });
    attempt("destination 0 column 1: d_src[1] is NULL", [](D, L, Cv, const u32** s, u32*) { s[1] = nullptr; });
    attempt("destination 0: NULL d_cols", [](D d, L, Cv, const u32**, u32*) { d[0].d_cols = (u32* const*)(uintptr_t)1; });
    attempt("destination 0: NULL limbs", [](D d, L, Cv, const u32**, u32*) { d[0].limbs = (const nx_part_limb*)(uintptr_t)1; });
    attempt("has the pointer of destination 0 column 0", [](D, L, Cv c, const u32**, u32*) { c[1] = c[0]; });
    attempt("has the pointer of", [](D d, L, Cv c, const u32**, u32*) { d[0].d_step = c[0]; });
    attempt("has the pointer of", [](D d, L, Cv, const u32**, u32*) { d[0].d_is_pad = d[0].d_step; });
    attempt("has the pointer of a source or class column", [&](D d, L, Cv, const u32**, u32*) { d[0].d_step = (u32*)s1.data(); });
    attempt("has the pointer of a source or class column", [&](D d, L, Cv, const u32**, u32*) { d[0].d_is_pad = (u32*)cls.data(); });
    nx_trace_partition_destroy(part);
    staged_release();
}

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const u32 sizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 5};
    const u32 ks[] = {1, 3, 40, 256};
    int i = 0;
    for (u32 n : sizes)
        for (u32 k : ks) {
            if (k == 256 && n > 257 && n != 3 * 1024 + 5) continue;       // 258 destinations a case: the large class counts at four sizes
            const Dist d = (Dist)(i % 10 == ALL_NONE ? UNIFORM : i % 10);
            run_case(n, k, d, i % 3, (i & 1) != 0, "n " + std::to_string(n) + " classes " + std::to_string(k) + " " + DIST_NAME[d]);
            i++;
        }
    for (int d = UNIFORM; d <= SPARSE; d++)
        for (u32 n : {1500u, 4u * 1024u + 1u})
            run_case(n, d == ALTERNATE ? 2 : 5, (Dist)d, 1, d & 1, std::string("skew ") + DIST_NAME[d] + " n " + std::to_string(n));
    // a class with exactly 2^k and 2^k + 1 steps: no padding at all, and almost nothing but padding
    run_case(512, 1, ONE_CLASS, 0, true, "exactly 2^9 steps");
    run_case(513, 1, ONE_CLASS, 0, true, "2^9 + 1 steps");
    refused_class(40);
    refused_class(0xFFFFFFFEu);
    refused_fill();
    printf("block cap %u\n%d failures, %d passed\n", (unsigned)CP_MAX_BLOCKS, n_fail, n_ok);
    return n_fail ? 1 : 0;
}
