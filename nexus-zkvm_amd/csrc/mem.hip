// The budget of a context's block allocator and the refusal injection behind the out-of-memory tests: the context options
// "mem.limit_bytes", "mem.cache_bytes", "mem.cached_bytes", "debug.fail_alloc" and "debug.alloc_count" (the context section of
// include/nexus_hip.h).  Host code only: every refusal is decided before a driver call, so nothing is ever
// launched with a pointer that was not handed out.  dev_alloc / dev_free themselves are in ctx.hip.
#include "internal.h"
#include <string.h>
#include <stdlib.h>

namespace nx {

int dev_alloc_admit(nx_ctx* ctx, size_t bytes, void** out) {
    ctx->alloc_count++;
    if (ctx->opt.debug_fail_alloc && ++ctx->fail_alloc_seen == (uint64_t)ctx->opt.debug_fail_alloc) {      // refused once, then the option is 0 again
        const int n = ctx->opt.debug_fail_alloc;
        ctx->opt.debug_fail_alloc = 0; ctx->fail_alloc_seen = 0;
        *out = nullptr;
        return set_err(ctx, NX_ERR_OOM, "debug.fail_alloc: request " + std::to_string(n) + " (" + std::to_string(bytes) + " bytes) refused");
    }
    const size_t limit = ctx->opt.mem_limit_bytes;
    if (limit && ctx->live_bytes + bytes > limit) {      // cached block or not: the live blocks alone would pass the budget
        *out = nullptr;
        return set_err(ctx, NX_ERR_OOM, "dev_alloc: " + std::to_string(bytes) + " bytes refused: " + std::to_string(ctx->live_bytes) + " live of a budget of " + std::to_string(limit) +
                                            " (mem.limit_bytes)");
    }
    return NX_OK;
}

// live + cached is what the context holds from the driver: the cache goes back first (what the hipErrorOutOfMemory retry of dev_alloc does)
void dev_alloc_make_room(nx_ctx* ctx, size_t bytes) {
    const size_t limit = ctx->opt.mem_limit_bytes;
    if (limit && ctx->cached_bytes && ctx->live_bytes + ctx->cached_bytes + bytes > limit) dev_cache_release(ctx);
}

static size_t env_bytes(const char* name, size_t dflt) { const char* e = getenv(name); return e && *e && *e != '-' ? (size_t)strtoull(e, nullptr, 10) : dflt; }
void mem_options_from_env(nx_options* o) {
    o->mem_limit_bytes = env_bytes("NX_MEM_LIMIT_BYTES", 0);
    o->mem_cache_bytes = env_bytes("NX_MEM_CACHE_BYTES", NX_MEM_CACHE_BYTES_DEFAULT);
    o->debug_fail_alloc = 0;                                        // armed per call, never from the environment
}

constexpr int64_t MEM_BYTES_MAX = (int64_t)1 << 62, FAIL_ALLOC_MAX = 1 << 30;
bool mem_option_set(nx_ctx* ctx, const char* name, int64_t value, int* rc) {
    const bool limit = !strcmp(name, "mem.limit_bytes"), cache = !strcmp(name, "mem.cache_bytes"), fail = !strcmp(name, "debug.fail_alloc");
    if (!strcmp(name, "debug.alloc_count") || !strcmp(name, "mem.cached_bytes")) { *rc = set_err(ctx, NX_ERR_ARG, std::string("nx_ctx_set_option: ") + name + " is read-only"); return true; }
    if (!limit && !cache && !fail) return false;
    if (value < 0 || value > (fail ? FAIL_ALLOC_MAX : MEM_BYTES_MAX)) { *rc = set_err(ctx, NX_ERR_ARG, std::string("nx_ctx_set_option: value out of range for ") + name); return true; }
    *rc = NX_OK;
    if (fail) { ctx->opt.debug_fail_alloc = (int)value; ctx->fail_alloc_seen = 0; return true; }      // the n-th request counted from here
    (limit ? ctx->opt.mem_limit_bytes : ctx->opt.mem_cache_bytes) = (size_t)value;
    // what the context holds beyond the new bound goes back to the driver now; live blocks stay (a limit below them refuses later requests only)
    const bool over = (ctx->opt.mem_limit_bytes && ctx->live_bytes + ctx->cached_bytes > ctx->opt.mem_limit_bytes) || ctx->cached_bytes > ctx->opt.mem_cache_bytes;
    if (over && ctx->cached_bytes) { NX_GUARD(ctx); dev_cache_release(ctx); }
    return true;
}
bool mem_option_get(const nx_ctx* ctx, const char* name, int64_t* value) {
    if (!strcmp(name, "mem.limit_bytes")) *value = (int64_t)ctx->opt.mem_limit_bytes;
    else if (!strcmp(name, "mem.cache_bytes")) *value = (int64_t)ctx->opt.mem_cache_bytes;
    else if (!strcmp(name, "mem.cached_bytes")) *value = (int64_t)ctx->cached_bytes;
    else if (!strcmp(name, "debug.fail_alloc")) *value = ctx->opt.debug_fail_alloc;
    else if (!strcmp(name, "debug.alloc_count")) *value = (int64_t)ctx->alloc_count;
    else return false;
    return true;
}

}  // namespace nx
