// C ABI of the host verifier (verifier.h): the nx_verifier_* session, the counterpart of nx_prover_*, and nx_verify_synth, the
// counterpart of nx_prove_synth.  No context, no device: these run in a process that cannot see a GPU.  (nx_verify_machine lives in
// machine.hip, next to the emitter of the machine's recorded AIR it rebuilds the components with.)
#include "verifier.h"
#include <new>
#include <stdio.h>

using namespace nxhip::verify;
using nxhip::Blake2sHash;

namespace {
void put_text(char* dst, size_t cap, const std::string& s) { if (dst && cap) snprintf(dst, cap, "%s", s.c_str()); }
}

extern "C" {

int nx_verifier_create(const nx_pcs_config* cfg, int hash_mode, nx_verifier** out) {
    if (!cfg || !out) return NX_ERR_ARG;
    *out = nullptr;
    if (!check_config(cfg, hash_mode).empty()) return NX_ERR_ARG;
    nx_verifier* v = new (std::nothrow) nx_verifier();
    if (!v) return NX_ERR_OOM;
    v->s.cfg = {cfg->pow_bits, cfg->log_blowup, cfg->n_queries, cfg->log_last_layer_degree_bound, cfg->fri_alpha_mode, cfg->log_constraint_degree, hash_mode};
    *out = v;
    return NX_OK;
}
void nx_verifier_destroy(nx_verifier* v) { delete v; }
const char* nx_verifier_last_error(const nx_verifier* v) { return v ? v->s.err.c_str() : "NULL verifier"; }

int nx_verifier_mix_u64(nx_verifier* v, uint64_t x) { if (!v) return NX_ERR_ARG; v->s.channel.mix_u64(x); return NX_OK; }
int nx_verifier_mix_felts(nx_verifier* v, const uint32_t* felts, uint32_t n) {
    if (!v) return NX_ERR_ARG;
    if (n && !felts) return v->s.fail(NX_ERR_ARG, "nx_verifier_mix_felts: NULL felts");
    v->s.channel.mix_u32s(felts, 4 * (size_t)n);
    return NX_OK;
}
int nx_verifier_draw_felt(nx_verifier* v, uint32_t out[4]) {
    if (!v) return NX_ERR_ARG;
    if (!out) return v->s.fail(NX_ERR_ARG, "nx_verifier_draw_felt: NULL output");
    nx::q_store(out, v->s.channel.draw_secure_felt());
    return NX_OK;
}
int nx_verifier_draw_felts(nx_verifier* v, uint32_t n, uint32_t* out) {
    if (!v) return NX_ERR_ARG;
    if (n && !out) return v->s.fail(NX_ERR_ARG, "nx_verifier_draw_felts: NULL output");
    for (uint32_t i = 0; i < n; i += 2) {       // two secure felts per draw of eight base felts, as Channel::draw_felts
        uint32_t f[8]; v->s.channel.draw_base_felts(f);
        memcpy(out + 4 * (size_t)i, f, 16);
        if (i + 1 < n) memcpy(out + 4 * (size_t)(i + 1), f + 4, 16);
    }
    return NX_OK;
}
int nx_verifier_channel_digest(const nx_verifier* v, uint8_t digest[32]) {
    if (!v || !digest) return NX_ERR_ARG;
    memcpy(digest, v->s.channel.digest.w, 32);
    return NX_OK;
}
int nx_verifier_tree_commit(nx_verifier* v, const uint8_t root[32], const uint32_t* log_sizes, uint32_t n_cols) {
    if (!v) return NX_ERR_ARG;
    try { return v->s.commit(root, log_sizes, n_cols); } catch (const std::bad_alloc&) { return v->s.fail(NX_ERR_OOM, "host allocation failed"); }
}
int nx_verifier_verify(nx_verifier* v, const nx_air_component* components, uint32_t n_components, const uint32_t* proof_words, size_t n_words) {
    if (!v) return NX_ERR_ARG;
    try {
        std::vector<Component> comps;
        const std::string e = components_from_abi(components, n_components, comps);
        if (!e.empty()) return v->s.fail(NX_ERR_ARG, "nx_verifier_verify: " + e);
        return v->s.verify(comps, proof_words, n_words);
    } catch (const std::bad_alloc&) { return v->s.fail(NX_ERR_OOM, "host allocation failed"); }
}

// The synthetic machine of nx_prove_synth: its transcript prefix (ad bytes, log sizes, the preprocessed and main roots out of the proof,
// one lookup element drawn, zero claimed sums, the interaction root) and its constraints at the out-of-domain point.
int nx_verify_synth(const nx_component_spec* comps, uint32_t n_comps, const nx_pcs_config* cfg, int hash_mode, const uint8_t* ad, size_t ad_len,
                    const uint32_t* proof_words, size_t n_words, char* err_text, size_t err_cap) {
    auto fail = [&](int rc, const std::string& s) { put_text(err_text, err_cap, s); return rc; };
    put_text(err_text, err_cap, "");
    if (!comps || !n_comps || !cfg || (ad_len && !ad) || (n_words && !proof_words)) return fail(NX_ERR_ARG, "nx_verify_synth: NULL argument or no components");
    try {
        { const std::string e = check_config(cfg, hash_mode); if (!e.empty()) return fail(NX_ERR_ARG, "nx_verify_synth: " + e); }
        for (uint32_t i = 0; i < n_comps; i++)
            if (comps[i].n_pre < 2 || comps[i].n_main < 2 || comps[i].log_size < 1 || comps[i].log_size > 28 || comps[i].n_pre > (1u << 20) || comps[i].n_main > (1u << 20) ||
                comps[i].n_inter > (1u << 20))
                return fail(NX_ERR_ARG, "nx_verify_synth: synthetic component needs n_pre >= 2, n_main >= 2, 1 <= log_size <= 28");
        // header (5 words), commitment count, four roots
        if (n_words < 6 + 32 || proof_words[0] != PROOF_MAGIC) return fail(NX_ERR_ARG, "proof words: not an NXP1 stream of a four-tree proof");
        if (proof_words[5] != 4) return fail(NX_ERR_VERIFY, "proof shape: the synthetic machine commits four trees");
        Session s;
        s.cfg = {cfg->pow_bits, cfg->log_blowup, cfg->n_queries, cfg->log_last_layer_degree_bound, cfg->fri_alpha_mode, cfg->log_constraint_degree, hash_mode};
        for (size_t i = 0; i < ad_len; i++) s.channel.mix_u64(ad[i]);
        for (uint32_t i = 0; i < n_comps; i++) s.channel.mix_u64(comps[i].log_size);
        std::vector<uint32_t> logs[3];
        std::vector<Component> air(n_comps);
        for (uint32_t i = 0; i < n_comps; i++) {
            const nx_component_spec& c = comps[i];
            Component& g = air[i];
            g.synth = true; g.log_size = c.log_size; g.log_cd = c.log_constraint_degree_bound; g.n_pre = c.n_pre; g.n_main = c.n_main; g.n_inter = c.n_inter;
            const uint32_t n[3] = {c.n_pre, c.n_main, c.n_inter};
            for (uint32_t t = 0; t < 3; t++)
                for (uint32_t k = 0; k < n[t]; k++) {
                    g.cols.push_back({t, (uint32_t)logs[t].size()});
                    g.masks.push_back(t == 1 && k < 2 ? std::vector<int>{0, 1} : std::vector<int>{0});
                    logs[t].push_back(c.log_size);
                }
        }
        const uint8_t* roots = (const uint8_t*)(proof_words + 6);
        int rc = s.commit(roots, logs[0].data(), (uint32_t)logs[0].size());
        if (rc == NX_OK) rc = s.commit(roots + 32, logs[1].data(), (uint32_t)logs[1].size());
        if (rc != NX_OK) return fail(rc, s.err);
        (void)s.channel.draw_secure_felt();                                  // the lookup element (machine.rs:239-240)
        s.channel.mix_felts(std::vector<nx::QM31>(n_comps, nx::q_zero()));   // claimed sums (machine.rs:262)
        rc = s.commit(roots + 64, logs[2].data(), (uint32_t)logs[2].size());
        if (rc != NX_OK) return fail(rc, s.err);
        rc = s.verify(air, proof_words, n_words);
        return rc == NX_OK ? NX_OK : fail(rc, s.err);
    } catch (const std::bad_alloc&) { return fail(NX_ERR_OOM, "host allocation failed"); }
}

}  // extern "C"
