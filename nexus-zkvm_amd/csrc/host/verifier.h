// The proof verifier of the product: `nexus_vm_prover::verify` (reference prover/src/lib.rs:26-33, prover/src/machine.rs:299-485,
// prover2/machine/src/verify.rs:28-143) from the point where the transcript prefix has been replayed — Stwo's core::verifier::verify,
// CommitmentSchemeVerifier::verify_values, FriVerifier and MerkleVerifier, restated from the published algorithm — over the NXP1 word
// stream the provers of this library write (prover.hip `serialize`).
//
// Host C++ only: KBs of hashing and a few hundred field operations whatever the trace size, so it needs no device and no context.  It
// compiles with a plain C++ compiler (tests/native/verifier_selftest.cpp builds it with the sanitizers) and with hipcc into the library.
// This is product code: it shares nothing with oracle/ (same rule as channel.h).
//
// UNTRUSTED INPUT.  The proof words come from outside.  Every count in the stream is bounded by the words that remain AND by what the
// statement (the committed column sizes, the components' masks, the configuration) says it must be before anything is allocated or
// indexed; a stream that cannot be parsed is NX_ERR_ARG, a parsed proof that fails a check is NX_ERR_VERIFY.  Nothing here throws on
// purpose, asserts or aborts.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "channel.h"
#include "../../../include/nexus_hip.h"

namespace nxhip {
namespace verify {

using namespace nx;

constexpr uint32_t PROOF_MAGIC = 0x3150584Eu;   // "NXP1"
constexpr uint32_t MAX_LDE_LOG = 30;            // circle_domain_index / half_odds_index hold up to here
constexpr uint32_t MAX_QUERIES = 1u << 12;
constexpr uint32_t MAX_LAST_LAYER_LOG = 16;

struct Config { uint32_t pow_bits, log_blowup, n_queries, log_last, fri_alpha_mode, log_constraint_degree; int hash_mode; };

// ---------------------------------------------------------------- the parsed proof ----------
struct Decommitment { const uint32_t* hashes = nullptr; size_t n_hashes = 0; const uint32_t* cols = nullptr; size_t n_cols = 0; };
struct FriLayerProof { std::vector<QM31> witness; Decommitment dec; Blake2sHash commitment; };
struct Proof {
    uint32_t pow_bits = 0, log_blowup = 0, n_queries = 0, log_last = 0;
    std::vector<Blake2sHash> commitments;
    std::vector<std::vector<std::vector<QM31>>> sampled;            // tree -> column -> mask
    std::vector<Decommitment> decommitments;
    std::vector<std::pair<const uint32_t*, size_t>> queried;       // views into the caller's words
    uint64_t nonce = 0;
    FriLayerProof first;
    std::vector<FriLayerProof> inner;
    std::vector<QM31> last_poly;
};

// What a proof of the statement must look like: per tree and column the number of sampled values; the counts that grow with the
// statement are compared as they are read, the others (witness lengths) are bounded by the remaining words only and checked exactly by
// the step that consumes them.
struct Shape { std::vector<std::vector<uint32_t>> n_samples; uint32_t n_inner_layers; uint32_t last_poly_len; };

struct Reader {
    const uint32_t* p; size_t n, i = 0; bool ok = true;
    Reader(const uint32_t* p_, size_t n_) : p(p_), n(n_) {}
    size_t left() const { return n - i; }
    uint32_t u() { if (i >= n) { ok = false; return 0; } return p[i++]; }
    // a count of items of `unit` words each: never more than the words that remain
    size_t count(size_t unit) { const uint32_t c = u(); if (!ok) return 0; if ((size_t)c > left() / unit) { ok = false; return 0; } return c; }
    const uint32_t* span(size_t words) { if (words > left()) { ok = false; return nullptr; } const uint32_t* r = p + i; i += words; return r; }
    Blake2sHash hash() { Blake2sHash h; memset(h.w, 0, 32); const uint32_t* s = span(8); if (s) memcpy(h.w, s, 32); return h; }
    QM31 felt() {   // canonical words only: a value >= p has no place in a proof (the prover never writes one)
        const uint32_t* s = span(4);
        if (!s) return q_zero();
        if (s[0] >= P || s[1] >= P || s[2] >= P || s[3] >= P) { ok = false; return q_zero(); }
        return qm(s[0], s[1], s[2], s[3]);
    }
};

enum { PARSE_OK = 0, PARSE_BAD = 1, PARSE_SHAPE = 2 };

inline void parse_decommitment(Reader& r, Decommitment& d) {
    d.n_hashes = r.count(8); d.hashes = r.span(8 * d.n_hashes);
    d.n_cols = r.count(1); d.cols = r.span(d.n_cols);
}
inline void parse_fri_layer(Reader& r, FriLayerProof& l) {
    const size_t n = r.count(4);
    l.witness.reserve(n);
    for (size_t k = 0; k < n && r.ok; k++) l.witness.push_back(r.felt());
    parse_decommitment(r, l.dec);
    l.commitment = r.hash();
}
inline int parse_proof(const uint32_t* w, size_t n, const Shape& shape, Proof& p, std::string& why) {
    Reader r(w, n);
    auto bad = [&](const char* s) { why = s; return (int)PARSE_BAD; };
    auto mis = [&](const std::string& s) { why = s; return (int)PARSE_SHAPE; };
    if (r.u() != PROOF_MAGIC || !r.ok) return bad("proof words: not an NXP1 stream");
    p.pow_bits = r.u(); p.log_blowup = r.u(); p.n_queries = r.u(); p.log_last = r.u();
    const size_t nt = r.count(8);
    if (!r.ok) return bad("proof words: truncated header");
    if (nt != shape.n_samples.size()) return mis("proof shape: " + std::to_string(nt) + " commitments, the statement has " + std::to_string(shape.n_samples.size()) + " trees");
    for (size_t t = 0; t < nt; t++) p.commitments.push_back(r.hash());
    p.sampled.resize(nt);
    for (size_t t = 0; t < nt; t++) {
        const size_t nc = r.count(1);
        if (!r.ok) return bad("proof words: truncated sampled values");
        if (nc != shape.n_samples[t].size()) return mis("proof shape: tree " + std::to_string(t) + " has sampled values of " + std::to_string(nc) + " columns, committed " + std::to_string(shape.n_samples[t].size()));
        p.sampled[t].resize(nc);
        for (size_t c = 0; c < nc; c++) {
            const size_t ns = r.count(4);
            if (!r.ok) return bad("proof words: truncated sampled values");
            if (ns != shape.n_samples[t][c]) return mis("proof shape: tree " + std::to_string(t) + " column " + std::to_string(c) + ": " + std::to_string(ns) + " sampled values, the mask has " + std::to_string(shape.n_samples[t][c]));
            p.sampled[t][c].reserve(ns);
            for (size_t s = 0; s < ns; s++) p.sampled[t][c].push_back(r.felt());
            if (!r.ok) return bad("proof words: truncated or non-canonical sampled value");
        }
    }
    p.decommitments.resize(nt);
    for (size_t t = 0; t < nt && r.ok; t++) parse_decommitment(r, p.decommitments[t]);
    p.queried.resize(nt);
    for (size_t t = 0; t < nt && r.ok; t++) { const size_t nv = r.count(1); p.queried[t] = {r.span(nv), nv}; }
    const uint32_t lo = r.u(), hi = r.u();
    p.nonce = (uint64_t)lo | ((uint64_t)hi << 32);
    if (!r.ok) return bad("proof words: truncated decommitments");
    parse_fri_layer(r, p.first);
    const size_t nl = r.count(1);
    if (!r.ok) return bad("proof words: truncated or non-canonical first FRI layer");
    if (nl != shape.n_inner_layers) return mis("proof shape: " + std::to_string(nl) + " inner FRI layers, the statement needs " + std::to_string(shape.n_inner_layers));
    p.inner.resize(nl);
    for (size_t l = 0; l < nl && r.ok; l++) parse_fri_layer(r, p.inner[l]);
    const size_t np = r.count(4);
    if (!r.ok) return bad("proof words: truncated or non-canonical FRI layer");
    if (np != shape.last_poly_len) return mis("proof shape: last-layer polynomial of " + std::to_string(np) + " coefficients, the degree bound is " + std::to_string(shape.last_poly_len));
    p.last_poly.reserve(np);
    for (size_t k = 0; k < np; k++) p.last_poly.push_back(r.felt());
    if (!r.ok) return bad("proof words: truncated or non-canonical last-layer polynomial");
    if (r.i != n) return bad("proof words: trailing words after the proof");
    return PARSE_OK;
}

// ---------------------------------------------------------------- Merkle ----------
// Blake2sMerkleHasher::hash_node under both node-hash rules (include/nexus_hip.h NX_HASH_*)
inline Blake2sHash hash_node(int mode, const Blake2sHash* left, const Blake2sHash* right, const uint32_t* vals, size_t n_vals) {
    Blake2sHash out;
    if (mode == NX_HASH_BLAKE2S) {
        Blake2sState s;
        if (left) { s.update(left->w, 32); s.update(right->w, 32); }
        if (n_vals) s.update(vals, n_vals * 4);
        s.finalize((uint8_t*)out.w);
        return out;
    }
    memset(out.w, 0, 32);                                  // raw compression chain from the zero state, t = f = 0, zero-padded blocks
    uint8_t block[64];
    if (left) { memcpy(block, left->w, 32); memcpy(block + 32, right->w, 32); Blake2sState::compress(out.w, block, 0, false); }
    for (size_t k = 0; k < n_vals; k += 16) {
        const size_t take = std::min<size_t>(16, n_vals - k);
        memset(block, 0, 64); memcpy(block, vals + k, 4 * take);
        Blake2sState::compress(out.w, block, 0, false);
    }
    return out;
}

typedef std::vector<std::vector<uint32_t>> QueriesByLog;   // index = log size (0 .. MAX_LDE_LOG), sorted distinct positions

// MerkleVerifier::verify of a mixed-degree tree: column_logs in commit order, `queried` = the values of the queried rows (layer by layer
// from the largest, row by row, column by column).  "" or the failing check.
inline std::string merkle_verify(int mode, const Blake2sHash& root, const std::vector<uint32_t>& column_logs, const QueriesByLog& queries,
                                 const uint32_t* queried, size_t n_queried, const Decommitment& d) {
    if (column_logs.empty()) {
        if (d.n_hashes || d.n_cols) return "witness too long";
        if (n_queried) return "too many queried values";
        const Blake2sHash h = hash_node(mode, nullptr, nullptr, nullptr, 0);
        return memcmp(h.w, root.w, 32) ? "Merkle root mismatch" : "";
    }
    uint32_t max_log = 0;
    std::vector<size_t> per_log(MAX_LDE_LOG + 1, 0);
    for (uint32_t l : column_logs) { if (l > MAX_LDE_LOG) return "column too large"; per_log[l]++; max_log = std::max(max_log, l); }
    size_t qv = 0, hw = 0, cw = 0;
    std::vector<std::pair<uint64_t, Blake2sHash>> below, here;       // nodes of the layer below / this layer that the walk knows
    std::vector<uint32_t> vals;
    static const std::vector<uint32_t> none;
    for (int log = (int)max_log; log >= 0; log--) {
        const size_t nc = per_log[log];
        const std::vector<uint32_t>& lq = (size_t)log < queries.size() ? queries[log] : none;
        const bool has_children = log < (int)max_log;
        vals.resize(nc);
        here.clear();
        size_t bi = 0, qi = 0;
        while (bi < below.size() || qi < lq.size()) {
            uint64_t node;
            if (bi < below.size() && qi < lq.size()) node = std::min<uint64_t>(below[bi].first >> 1, lq[qi]);
            else node = bi < below.size() ? below[bi].first >> 1 : lq[qi];
            Blake2sHash l, r;
            if (has_children) {
                for (int side = 0; side < 2; side++) {
                    Blake2sHash& dst = side ? r : l;
                    if (bi < below.size() && below[bi].first == 2 * node + side) dst = below[bi++].second;
                    else { if (hw >= d.n_hashes) return "hash witness too short"; memcpy(dst.w, d.hashes + 8 * hw++, 32); }
                }
            }
            const uint32_t* src;
            if (qi < lq.size() && lq[qi] == node) {
                qi++;
                if (nc > n_queried - qv) return "too few queried values";
                src = queried + qv; qv += nc;
            } else {
                if (nc > d.n_cols - cw) return "column witness too short";
                src = d.cols + cw; cw += nc;
            }
            if (nc) memcpy(vals.data(), src, 4 * nc);
            here.push_back({node, hash_node(mode, has_children ? &l : nullptr, has_children ? &r : nullptr, vals.data(), nc)});
        }
        below.swap(here);
    }
    if (hw != d.n_hashes || cw != d.n_cols) return "witness too long";
    if (qv != n_queried) return "too many queried values";
    if (below.size() != 1 || memcmp(below[0].second.w, root.w, 32)) return "Merkle root mismatch";
    return "";
}

// ---------------------------------------------------------------- points and domains ----------
inline QPt random_point(Blake2sChannel& ch) {                 // CirclePoint::get_random_point
    const QM31 t = ch.draw_secure_felt(), t2 = q_sqr(t), inv = q_inv(q_add(t2, q_one()));
    QPt p; p.x = q_mul(q_sub(q_one(), t2), inv); p.y = q_mul(q_add(t, t), inv);
    return p;
}
inline QM31 coset_vanishing(uint32_t log_size, QPt p) { QM31 x = p.x; for (uint32_t k = 1; k < log_size; k++) x = q_double_x(x); return x; }
inline QPt mask_point(QPt oods, uint32_t log_size, int offset) {     // oods + offset trace steps
    if (offset == 0) return oods;
    const int64_t idx = ((int64_t)offset * ((int64_t)1 << (31 - log_size))) & 0x7fffffffLL;
    const Pt s = pt_from_index((u32)idx);
    QPt q; q.x = q_from_m(s.x); q.y = q_from_m(s.y);
    return qpt_add(oods, q);
}
inline bool qpt_eq(const QPt& a, const QPt& b) { return q_eq(a.x, b.x) && q_eq(a.y, b.y); }
inline Pt lde_point(uint32_t log, uint32_t pos) { return pt_from_index(circle_domain_index((int)log, bitrev(pos, (int)log))); }
inline u32 line_x(uint32_t log, uint32_t pos) { return pt_from_index(half_odds_index((int)log, bitrev(pos, (int)log))).x; }
inline QM31 partial_evals(const QM31 e[4]) {                    // c0 + c1 i + c2 u + c3 iu
    QM31 r = e[0];
    r = q_add(r, q_mul(e[1], qm(0, 1, 0, 0)));
    r = q_add(r, q_mul(e[2], qm(0, 0, 1, 0)));
    return q_add(r, q_mul(e[3], qm(0, 0, 0, 1)));
}
// one inverse-butterfly fold of a pair: (f0 + f1) + alpha (f0 - f1) / t
inline QM31 fold_pair(QM31 f0, QM31 f1, u32 t, QM31 alpha) { return q_add(q_add(f0, f1), q_mul(alpha, q_mul_m(q_sub(f0, f1), m_inv(t)))); }

// ---------------------------------------------------------------- the statement's AIR ----------
// A component as nx_prover_prove takes it, or (synth) the synthetic machine's component of nx_prove_synth, whose constraints the product
// otherwise has only as a device kernel (constraints.hip synth_constraints_kernel).
struct Component {
    uint32_t log_size = 0, log_cd = 0;
    std::vector<std::pair<uint32_t, uint32_t>> cols;      // component column -> (tree, column in the tree)
    std::vector<std::vector<int>> masks;
    bool synth = false; uint32_t n_pre = 0, n_main = 0, n_inter = 0;
    const nx_cinstr* prog = nullptr; uint32_t n_instr = 0, n_regs = 0; const uint32_t* econsts = nullptr; uint32_t n_econsts = 0, n_constraints = 0;
};

inline bool synth_free(uint32_t k) { return (k % 16) < 2; }

// "" when the program only names registers, columns and constants that exist (what nx_air_compile checks on the proving side)
inline std::string check_program(const Component& c) {
    if (c.n_instr && !c.prog) return "NULL program";
    if (c.n_regs == 0 || c.n_regs > 4096) return "register count out of range";
    const uint32_t n_cols = (uint32_t)c.cols.size();
    uint32_t n_c = 0;
    for (uint32_t i = 0; i < c.n_instr; i++) {
        const nx_cinstr& in = c.prog[i];
        auto reg = [&](uint32_t rg, uint32_t width) { return rg <= c.n_regs && width <= c.n_regs - rg; };
        bool ok;
        switch (in.op) {
        case NX_C_LOAD: ok = reg(in.dst, 1) && in.a < n_cols; break;
        case NX_C_CONST: ok = reg(in.dst, 1) && in.a < P; break;
        case NX_C_ADD: case NX_C_SUB: case NX_C_MUL: ok = reg(in.dst, 1) && reg(in.a, 1) && reg(in.b, 1); break;
        case NX_C_NEG: ok = reg(in.dst, 1) && reg(in.a, 1); break;
        case NX_C_CONSTE: ok = reg(in.dst, 4) && in.a < c.n_econsts; break;
        case NX_C_ADDE: case NX_C_SUBE: case NX_C_MULE: ok = reg(in.dst, 4) && reg(in.a, 4) && reg(in.b, 4); break;
        case NX_C_MULEB: case NX_C_ADDEB: ok = reg(in.dst, 4) && reg(in.a, 4) && reg(in.b, 1); break;
        case NX_C_LOADE: ok = reg(in.dst, 4) && in.a < n_cols && n_cols - in.a >= 4; break;
        case NX_C_CONSTRAINT_B: ok = reg(in.a, 1); n_c++; break;
        case NX_C_CONSTRAINT_E: ok = reg(in.a, 4); n_c++; break;
        default: ok = false;
        }
        if (!ok) return "malformed instruction " + std::to_string(i);
        if (in.op == NX_C_LOAD || in.op == NX_C_LOADE)
            for (uint32_t j = 0; j < (in.op == NX_C_LOADE ? 4u : 1u); j++) {
                const std::vector<int>& m = c.masks[in.a + j];
                if (std::find(m.begin(), m.end(), (int)(int32_t)in.b) == m.end()) return "LOAD at an offset missing from the column's mask";
            }
    }
    for (uint32_t k = 0; k < c.n_econsts; k++) for (int q = 0; q < 4; q++) if (c.econsts[4 * k + q] >= P) return "secure constant not canonical";
    if (n_c != c.n_constraints) return "constraint count mismatch";
    return "";
}

struct Tree { Blake2sHash root; std::vector<uint32_t> logs; };

// The AIR against the committed trees: the union of mask offsets per committed column (first-appearance order, as the prover samples
// them) or the reason the components do not describe these trees.
inline std::string bind_components(const std::vector<Component>& comps, const std::vector<Tree>& trees, const Config& cfg,
                                   std::vector<std::vector<std::vector<int>>>& offs, uint32_t* composition_log) {
    if (trees.empty()) return "at least one trace tree must be committed first";
    if (comps.empty()) return "no components";
    offs.assign(trees.size(), {});
    std::vector<std::vector<char>> claimed(trees.size());
    for (size_t t = 0; t < trees.size(); t++) { offs[t].resize(trees[t].logs.size()); claimed[t].assign(trees[t].logs.size(), 0); }
    *composition_log = 0;
    for (const Component& c : comps) {
        if (c.log_cd > cfg.log_constraint_degree) return "a component's log_constraint_degree_bound exceeds the config's log_constraint_degree";
        if (c.log_size < 1 || c.log_size > 28) return "component log_size outside 1 .. 28";
        if (c.masks.size() != c.cols.size()) return "one mask list per component column required";
        for (size_t k = 0; k < c.cols.size(); k++) {
            const uint32_t t = c.cols[k].first, i = c.cols[k].second;
            if (t >= trees.size() || i >= trees[t].logs.size()) return "component column outside the committed trees";
            if (trees[t].logs[i] != c.log_size) return "component column of a different log size than the component";
            claimed[t][i] = 1;
            for (int o : c.masks[k]) if (std::find(offs[t][i].begin(), offs[t][i].end(), o) == offs[t][i].end()) offs[t][i].push_back(o);
        }
        if (c.synth) { if (c.n_pre < 2 || c.n_main < 2) return "synthetic component needs n_pre >= 2 and n_main >= 2"; }
        else { const std::string e = check_program(c); if (!e.empty()) return "recorded AIR: " + e; }
        *composition_log = std::max(*composition_log, c.log_size + (c.log_cd ? c.log_cd : cfg.log_constraint_degree));
    }
    for (size_t t = 0; t < trees.size(); t++) for (char x : claimed[t]) if (!x) return "a committed column is claimed by no component";
    if (*composition_log + cfg.log_blowup > MAX_LDE_LOG) return "composition polynomial domain too large";
    return "";
}

// components().eval_composition_polynomial_at_point: every recorded program runs once, over QM31, on the sampled mask values
inline QM31 eval_composition(const std::vector<Component>& comps, const std::vector<std::vector<std::vector<int>>>& offs, QPt point,
                             const std::vector<std::vector<std::vector<QM31>>>& sv, QM31 rc) {
    QM31 acc = q_zero();
    std::vector<QM31> R;
    for (const Component& c : comps) {
        const QM31 di = q_inv(coset_vanishing(c.log_size, point));
        auto add = [&](QM31 v) { acc = q_add(q_mul(acc, rc), q_mul(di, v)); };
        auto sampled = [&](uint32_t col, int off) {
            const uint32_t t = c.cols[col].first, i = c.cols[col].second;
            const std::vector<int>& o = offs[t][i];
            const size_t k = std::find(o.begin(), o.end(), off) - o.begin();      // present: bind_components put every mask offset there
            return sv[t][i][k];
        };
        if (c.synth) {
            const uint32_t M0 = c.n_pre, I0 = c.n_pre + c.n_main;
            auto M = [&](uint32_t k, int s = 0) { return sampled(M0 + k, s); };
            auto I = [&](uint32_t k) { return sampled(I0 + k, 0); };
            const QM31 not_last = q_sub(q_one(), sampled(1, 0));
            add(q_mul(q_sub(q_sub(M(0, 1), M(0)), q_one()), not_last));
            add(q_mul(q_sub(q_sub(M(1, 1), M(1)), M(0)), not_last));
            for (uint32_t k = 2; k < c.n_main; k++) if (!synth_free(k)) add(q_sub(q_sub(M(k), q_sqr(M(k - 1))), q_sqr(M(k - 2))));
            for (uint32_t k = 0; k < c.n_inter; k++) if (!synth_free(k)) add(q_sub(q_sub(I(k), q_sqr(I(k - 1))), q_sqr(I(k - 2))));
            continue;
        }
        // one QM31 per register index: a base-field register holds its value embedded, a secure one lives at its first index
        R.assign(c.n_regs, q_zero());
        for (uint32_t pc = 0; pc < c.n_instr; pc++) {
            const nx_cinstr& in = c.prog[pc];
            switch (in.op) {
            case NX_C_LOAD: R[in.dst] = sampled(in.a, (int)(int32_t)in.b); break;
            case NX_C_CONST: R[in.dst] = q_from_m(in.a); break;
            case NX_C_ADD: case NX_C_ADDE: case NX_C_ADDEB: R[in.dst] = q_add(R[in.a], R[in.b]); break;
            case NX_C_SUB: case NX_C_SUBE: R[in.dst] = q_sub(R[in.a], R[in.b]); break;
            case NX_C_MUL: case NX_C_MULE: case NX_C_MULEB: R[in.dst] = q_mul(R[in.a], R[in.b]); break;
            case NX_C_NEG: R[in.dst] = q_neg(R[in.a]); break;
            case NX_C_CONSTE: R[in.dst] = q_load(c.econsts + 4 * (size_t)in.a); break;
            case NX_C_LOADE: { QM31 e[4]; for (uint32_t j = 0; j < 4; j++) e[j] = sampled(in.a + j, (int)(int32_t)in.b); R[in.dst] = partial_evals(e); break; }
            case NX_C_CONSTRAINT_B: case NX_C_CONSTRAINT_E: add(R[in.a]); break;
            default: break;
            }
        }
    }
    return acc;
}

// ---------------------------------------------------------------- DEEP quotients at one row ----------
struct SampleBatch { QPt point; std::vector<std::pair<size_t, QM31>> cols; };      // (index in the size group's row, sampled value)
struct LineCoeffs { QM31 a, b, c; };

inline QM31 row_quotient(const std::vector<SampleBatch>& batches, const std::vector<std::vector<LineCoeffs>>& lines, const std::vector<QM31>& batch_coeff,
                         const uint32_t* row, Pt dp) {
    QM31 acc = q_zero();
    for (size_t b = 0; b < batches.size(); b++) {
        const QPt& p = batches[b].point;
        // (Re(p.x) - d.x) Im(p.y) - (Re(p.y) - d.y) Im(p.x) over CM31
        const CM31 den = c_sub(c_mul(c_sub(p.x.a, cm(dp.x, 0)), p.y.b), c_mul(c_sub(p.y.a, cm(dp.y, 0)), p.x.b));
        const CM31 den_inv = c_inv(den);
        QM31 num = q_zero();
        for (size_t k = 0; k < batches[b].cols.size(); k++) {
            const LineCoeffs& l = lines[b][k];
            num = q_add(num, q_sub(q_mul_m(l.c, row[batches[b].cols[k].first]), q_add(q_mul_m(l.a, dp.y), l.b)));
        }
        acc = q_add(q_mul(acc, batch_coeff[b]), q_mul_c(num, den_inv));
    }
    return acc;
}

// queries folded n times: positions >> n, duplicates (adjacent after the shift) dropped
inline std::vector<uint32_t> fold_queries(const std::vector<uint32_t>& q, uint32_t n) {
    std::vector<uint32_t> r;
    for (uint32_t p : q) { const uint32_t f = n >= 32 ? 0 : p >> n; if (r.empty() || r.back() != f) r.push_back(f); }
    return r;
}

// ---------------------------------------------------------------- core::verifier::verify ----------
// From the point where the trace trees are in the transcript.  Returns NX_OK, NX_ERR_VERIFY or NX_ERR_ARG; `why` names the check.
inline int verify_core(Blake2sChannel& ch, const Config& cfg, const std::vector<Tree>& trace_trees, const std::vector<Component>& comps,
                       const uint32_t* words, size_t n_words, std::string& why) {
    auto refuse = [&](const std::string& s) { why = s; return NX_ERR_VERIFY; };
    const size_t T = trace_trees.size();
    std::vector<std::vector<std::vector<int>>> offs;
    uint32_t clog = 0;
    { const std::string e = bind_components(comps, trace_trees, cfg, offs, &clog); if (!e.empty()) { why = e; return NX_ERR_ARG; } }
    if (!words && n_words) { why = "NULL proof words"; return NX_ERR_ARG; }

    // the trees of the statement plus the composition polynomial's; distinct LDE sizes, descending: FRI's circle columns
    std::vector<std::vector<uint32_t>> lde(T + 1);
    std::vector<char> has_log(MAX_LDE_LOG + 1, 0);
    for (size_t t = 0; t < T; t++) for (uint32_t l : trace_trees[t].logs) { lde[t].push_back(l + cfg.log_blowup); has_log[l + cfg.log_blowup] = 1; }
    lde[T].assign(4, clog + cfg.log_blowup); has_log[clog + cfg.log_blowup] = 1;
    std::vector<uint32_t> col_logs;
    for (int l = (int)MAX_LDE_LOG; l >= 0; l--) if (has_log[l]) col_logs.push_back((uint32_t)l);
    const uint32_t max_log = col_logs[0], last_log = cfg.log_last + cfg.log_blowup;

    Shape shape;
    shape.n_samples.resize(T + 1);
    for (size_t t = 0; t < T; t++) for (auto& o : offs[t]) shape.n_samples[t].push_back((uint32_t)o.size());
    shape.n_samples[T].assign(4, 1);
    shape.n_inner_layers = max_log - 1 > last_log ? max_log - 1 - last_log : 0;
    shape.last_poly_len = 1u << cfg.log_last;
    Proof proof;
    {
        const int pr = parse_proof(words, n_words, shape, proof, why);
        if (pr == PARSE_BAD) return NX_ERR_ARG;
        if (pr == PARSE_SHAPE) return NX_ERR_VERIFY;
    }
    if (proof.pow_bits != cfg.pow_bits || proof.log_blowup != cfg.log_blowup || proof.n_queries != cfg.n_queries || proof.log_last != cfg.log_last)
        return refuse("proof shape: the proof was made under another PCS configuration");
    for (size_t t = 0; t < T; t++)
        if (memcmp(proof.commitments[t].w, trace_trees[t].root.w, 32)) return refuse("tree " + std::to_string(t) + ": the proof's commitment is not the committed root");

    const QM31 random_coeff = ch.draw_secure_felt();
    ch.mix_root(proof.commitments[T]);
    const QPt oods = random_point(ch);
    {
        QM31 ce[4]; for (int k = 0; k < 4; k++) ce[k] = proof.sampled[T][k][0];
        if (!q_eq(partial_evals(ce), eval_composition(comps, offs, oods, proof.sampled, random_coeff)))
            return refuse("composition polynomial: the out-of-domain value does not match the sampled values");
    }
    { std::vector<QM31> flat; for (auto& t : proof.sampled) for (auto& c : t) for (auto& v : c) flat.push_back(v); ch.mix_felts(flat); }
    const QM31 q_coeff = ch.draw_secure_felt();

    // FriVerifier::commit: the commit phase replayed on the channel
    ch.mix_root(proof.first.commitment);
    const QM31 first_alpha = ch.draw_secure_felt();
    std::vector<QM31> inner_alpha;
    for (auto& l : proof.inner) { ch.mix_root(l.commitment); inner_alpha.push_back(ch.draw_secure_felt()); }
    {   // the prover mixed the coefficients in LinePoly's storage order (bit-reversed)
        std::vector<QM31> m(proof.last_poly.size());
        for (size_t i = 0; i < m.size(); i++) m[i] = proof.last_poly[bitrev((u32)i, (int)cfg.log_last)];
        ch.mix_felts(m);
    }
    {   // proof of work: trailing zero bits of the first 16 digest bytes (little-endian u128) after mixing the nonce
        Blake2sChannel c2 = ch; c2.mix_u64(proof.nonce);
        uint32_t tz = 128;
        for (int i = 0; i < 4; i++) if (c2.digest.w[i]) { tz = 32 * i + (uint32_t)__builtin_ctz(c2.digest.w[i]); break; }
        if (tz < cfg.pow_bits) return refuse("proof of work");
    }
    ch.mix_u64(proof.nonce);

    // Queries::generate and their folds per column size
    std::vector<uint32_t> queries;
    {
        const uint32_t mask = (uint32_t)(((uint64_t)1 << max_log) - 1);
        uint32_t cnt = 0;
        while (cnt < cfg.n_queries) {
            uint32_t w[8]; ch.draw_u32s(w);
            for (int i = 0; i < 8 && cnt < cfg.n_queries; i++, cnt++) queries.push_back(w[i] & mask);
        }
        std::sort(queries.begin(), queries.end());
        queries.erase(std::unique(queries.begin(), queries.end()), queries.end());
    }
    QueriesByLog qpos(MAX_LDE_LOG + 1);
    for (uint32_t l : col_logs) qpos[l] = fold_queries(queries, max_log - l);

    for (size_t t = 0; t <= T; t++) {
        const std::string e = merkle_verify(cfg.hash_mode, proof.commitments[t], lde[t], qpos, proof.queried[t].first, proof.queried[t].second, proof.decommitments[t]);
        if (!e.empty()) return refuse("tree " + std::to_string(t) + ": " + e);
    }

    // fri_answers: the DEEP quotient of every size group at its queried rows
    std::vector<std::vector<QM31>> answers(col_logs.size());
    {
        std::vector<size_t> cursor(T + 1, 0);
        std::vector<uint32_t> row;
        for (size_t g = 0; g < col_logs.size(); g++) {
            const uint32_t L = col_logs[g];
            std::vector<SampleBatch> batches;
            std::vector<size_t> in_tree(T + 1, 0);
            size_t member = 0;
            for (size_t t = 0; t <= T; t++) for (size_t c = 0; c < lde[t].size(); c++) {
                if (lde[t][c] != L) continue;
                in_tree[t]++;
                for (size_t k = 0; k < proof.sampled[t][c].size(); k++) {
                    const QPt pt = t == T ? oods : mask_point(oods, lde[t][c] - cfg.log_blowup, offs[t][c][k]);
                    size_t b = 0;
                    while (b < batches.size() && !qpt_eq(batches[b].point, pt)) b++;
                    if (b == batches.size()) { SampleBatch nb; nb.point = pt; batches.push_back(nb); }
                    batches[b].cols.push_back({member, proof.sampled[t][c][k]});
                }
                member++;
            }
            std::vector<std::vector<LineCoeffs>> lines(batches.size());
            std::vector<QM31> batch_coeff(batches.size());
            for (size_t b = 0; b < batches.size(); b++) {
                QM31 alpha = q_one();
                const QPt& p = batches[b].point;
                const QM31 c = q_sub(q_conj(p.y), p.y);
                for (auto& cv : batches[b].cols) {
                    alpha = q_mul(alpha, q_coeff);
                    const QM31 a = q_sub(q_conj(cv.second), cv.second);
                    const QM31 bb = q_sub(q_mul(cv.second, c), q_mul(a, p.y));
                    lines[b].push_back({q_mul(alpha, a), q_mul(alpha, bb), q_mul(alpha, c)});
                }
                batch_coeff[b] = alpha;                                   // q_coeff ^ (columns of the batch)
            }
            row.resize(member);
            for (uint32_t q : qpos[L]) {
                size_t at = 0;
                for (size_t t = 0; t <= T; t++) for (size_t k = 0; k < in_tree[t]; k++) {
                    if (cursor[t] >= proof.queried[t].second) return refuse("tree " + std::to_string(t) + ": too few queried values");
                    row[at++] = proof.queried[t].first[cursor[t]++];
                }
                answers[g].push_back(row_quotient(batches, lines, batch_coeff, row.data(), lde_point(L, q)));
            }
        }
    }

    // ---- FriVerifier::decommit ----
    // A layer's pairs: the positions 2k, 2k + 1 of every queried k, values from the layer below where a query supplies them, else from the witness
    struct Pairs { std::vector<uint32_t> index; std::vector<QM31> v0, v1; std::vector<uint32_t> positions; std::vector<uint32_t> flat; };
    auto rebuild = [](const std::vector<uint32_t>& q, const std::vector<QM31>& known, const std::vector<QM31>& witness, size_t* wi, Pairs* out) -> bool {
        size_t i = 0;
        while (i < q.size()) {
            const uint32_t pair = q[i] >> 1;
            QM31 pv[2];
            for (uint32_t side = 0; side < 2; side++) {
                const uint32_t pos = 2 * pair + side;
                if (i < q.size() && q[i] == pos) pv[side] = known[i++];
                else { if (*wi >= witness.size()) return false; pv[side] = witness[(*wi)++]; }
                out->positions.push_back(pos);
                uint32_t w4[4]; q_store(w4, pv[side]); out->flat.insert(out->flat.end(), w4, w4 + 4);
            }
            out->index.push_back(pair); out->v0.push_back(pv[0]); out->v1.push_back(pv[1]);
        }
        return true;
    };
    std::vector<Pairs> circle(col_logs.size());
    {
        size_t wi = 0;
        QueriesByLog pos(MAX_LDE_LOG + 1);
        std::vector<uint32_t> mlogs, flat;
        for (size_t g = 0; g < col_logs.size(); g++) {
            if (!rebuild(qpos[col_logs[g]], answers[g], proof.first.witness, &wi, &circle[g])) return refuse("FRI first layer: too few witness evaluations");
            pos[col_logs[g]] = circle[g].positions;
            for (int k = 0; k < 4; k++) mlogs.push_back(col_logs[g]);
            flat.insert(flat.end(), circle[g].flat.begin(), circle[g].flat.end());
        }
        if (wi != proof.first.witness.size()) return refuse("FRI first layer: too many witness evaluations");
        const std::string e = merkle_verify(cfg.hash_mode, proof.first.commitment, mlogs, pos, flat.data(), flat.size(), proof.first.dec);
        if (!e.empty()) return refuse("FRI first layer: " + e);
    }
    std::vector<uint32_t> lq = fold_queries(queries, 1);
    std::vector<QM31> lvals(lq.size(), q_zero());
    size_t next_circle = 0;
    QM31 prev_alpha = first_alpha;
    uint32_t layer_log = max_log - 1;
    for (size_t li = 0; li < proof.inner.size(); li++) {
        // the circle columns of this size fold into the line first (fold_circle_into_line)
        while (next_circle < col_logs.size() && col_logs[next_circle] - 1 == layer_log) {
            const QM31 a = cfg.fri_alpha_mode == NX_FRI_ALPHA_PREV ? prev_alpha : first_alpha, a2 = q_sqr(a);
            const Pairs& sp = circle[next_circle];
            const uint32_t L = col_logs[next_circle];
            if (sp.index != lq) return refuse("FRI first layer: query positions do not line up with layer " + std::to_string(li));
            for (size_t i = 0; i < lq.size(); i++)
                lvals[i] = q_add(q_mul(lvals[i], a2), fold_pair(sp.v0[i], sp.v1[i], lde_point(L, sp.index[i] << 1).y, a));
            next_circle++;
        }
        const FriLayerProof& lp = proof.inner[li];
        Pairs pr; size_t wi = 0;
        if (!rebuild(lq, lvals, lp.witness, &wi, &pr)) return refuse("FRI layer " + std::to_string(li) + ": too few witness evaluations");
        if (wi != lp.witness.size()) return refuse("FRI layer " + std::to_string(li) + ": too many witness evaluations");
        QueriesByLog pos(MAX_LDE_LOG + 1); pos[layer_log] = pr.positions;
        const std::string e = merkle_verify(cfg.hash_mode, lp.commitment, std::vector<uint32_t>(4, layer_log), pos, pr.flat.data(), pr.flat.size(), lp.dec);
        if (!e.empty()) return refuse("FRI layer " + std::to_string(li) + ": " + e);
        std::vector<QM31> nv(pr.index.size());
        for (size_t i = 0; i < pr.index.size(); i++) nv[i] = fold_pair(pr.v0[i], pr.v1[i], line_x(layer_log, pr.index[i] << 1), inner_alpha[li]);
        lq = pr.index; lvals.swap(nv); prev_alpha = inner_alpha[li];
        layer_log--;
    }
    if (next_circle != col_logs.size()) return refuse("FRI: a committed column is smaller than the last layer");
    // the last layer: the polynomial of degree < 2^log_last at every remaining query
    for (size_t i = 0; i < lq.size(); i++) {
        QM31 x = q_from_m(line_x(layer_log, lq[i]));
        std::vector<QM31> d(cfg.log_last);
        for (uint32_t k = 0; k < cfg.log_last; k++) { d[k] = x; x = q_double_x(x); }
        QM31 v = q_zero();
        for (size_t j = 0; j < proof.last_poly.size(); j++) {     // coefficient j multiplies the doublings its set bits name
            QM31 term = proof.last_poly[j];
            for (uint32_t k = 0; k < cfg.log_last; k++) if ((j >> k) & 1) term = q_mul(term, d[k]);
            v = q_add(v, term);
        }
        if (!q_eq(v, lvals[i])) return refuse("FRI last layer: fold mismatch at query " + std::to_string(i));
    }
    return NX_OK;
}

// ---------------------------------------------------------------- the session ----------
// CommitmentSchemeVerifier + Blake2sChannel, mirroring the prover session one to one: the caller replays the transcript prefix
// (mix, commit a root with its column sizes, draw) and verify() runs core::verifier::verify.
struct Session {
    Config cfg; Blake2sChannel channel; std::vector<Tree> trees; std::string err;
    bool verified = false; Blake2sChannel pre_channel;
    int fail(int rc, const std::string& s) { err = s; return rc; }
    int commit(const uint8_t root[32], const uint32_t* logs, uint32_t n) {
        if (!root || (n && !logs)) return fail(NX_ERR_ARG, "nx_verifier_tree_commit: NULL argument");
        if (verified) return fail(NX_ERR_ARG, "nx_verifier_tree_commit: the session has verified a proof already");
        Tree t; memcpy(t.root.w, root, 32);
        for (uint32_t i = 0; i < n; i++) {
            if (logs[i] < 1 || logs[i] > 28 || logs[i] + cfg.log_blowup > MAX_LDE_LOG) return fail(NX_ERR_ARG, "nx_verifier_tree_commit: column log size outside 1 .. 28");
            t.logs.push_back(logs[i]);
        }
        channel.mix_root(t.root);
        trees.push_back(std::move(t));
        return NX_OK;
    }
    // After an accepted proof the channel is the transcript's final state, as after nx_prover_prove; a later call starts again from the
    // state the first one found, and a refused one puts that state back at once: verifying again gives the same answer.
    int verify(const std::vector<Component>& comps, const uint32_t* words, size_t n_words) {
        if (!verified) pre_channel = channel; else channel = pre_channel;
        std::string why;
        int rc;
        try { rc = verify_core(channel, cfg, trees, comps, words, n_words, why); }
        catch (const std::bad_alloc&) { rc = NX_ERR_OOM; why = "host allocation failed"; }
        verified = rc == NX_OK;
        if (rc != NX_OK) { channel = pre_channel; err = why; }
        return rc;
    }
};

inline std::string check_config(const nx_pcs_config* c, int hash_mode) {
    if (c->log_blowup < 1 || c->log_blowup > 16) return "log_blowup outside 1 .. 16";
    if (c->log_constraint_degree < 1 || c->log_constraint_degree > 2) return "log_constraint_degree must be 1 or 2";
    if (c->n_queries < 1 || c->n_queries > MAX_QUERIES) return "n_queries outside 1 .. 4096";
    if (c->log_last_layer_degree_bound > MAX_LAST_LAYER_LOG) return "log_last_layer_degree_bound too large";
    if (c->pow_bits > 128) return "pow_bits above 128";
    if (c->fri_alpha_mode != NX_FRI_ALPHA_PREV && c->fri_alpha_mode != NX_FRI_ALPHA_FIRST) return "unknown fri_alpha_mode";
    if (hash_mode != NX_HASH_BLAKE2S && hash_mode != NX_HASH_BLAKE2S_RAW0) return "unknown hash_mode";
    return "";
}

// nx_air_component array -> components (the pointers stay the caller's)
inline std::string components_from_abi(const nx_air_component* a, uint32_t n, std::vector<Component>& out) {
    if (n && !a) return "NULL components";
    for (uint32_t i = 0; i < n; i++) {
        const nx_air_component& u = a[i];
        if ((u.n_instr && !u.program) || (u.n_cols && (!u.col_tree || !u.col_index || !u.mask_count)) || (u.n_econsts && !u.econsts)) return "NULL pointer in a component";
        if (u.n_cols > (1u << 24) || u.n_instr > (1u << 28) || u.n_econsts > (1u << 24)) return "component too large";
        Component c;
        c.log_size = u.log_size; c.log_cd = u.log_constraint_degree_bound;
        c.prog = u.program; c.n_instr = u.n_instr; c.n_regs = u.n_regs; c.econsts = u.econsts; c.n_econsts = u.n_econsts; c.n_constraints = u.n_constraints;
        size_t m = 0;
        for (uint32_t k = 0; k < u.n_cols; k++) {
            if (u.mask_count[k] > 64) return "more than 64 mask offsets on a column";
            if (u.mask_count[k] && !u.mask_offsets) return "mask_offsets is NULL but a column has a nonzero mask_count";
            c.cols.push_back({u.col_tree[k], u.col_index[k]});
            std::vector<int> o;
            for (uint32_t j = 0; j < u.mask_count[k]; j++) o.push_back((int)u.mask_offsets[m++]);
            c.masks.push_back(std::move(o));
        }
        out.push_back(std::move(c));
    }
    return "";
}

}  // namespace verify
}  // namespace nxhip

struct nx_verifier { nxhip::verify::Session s; };
