// Memory-checking columns on the device: for every access, what the previous access to the same address left behind, when every access
// knows in advance what it leaves (registers, program memory, RAM by load/store).  The kernels and the host driver are access_history.cuh's,
// in the instantiation without block streams, rules and chained columns.
#include "internal.h"
#include <algorithm>
#include <string.h>
#include <string>
#include <type_traits>

namespace nx {
#include "access_history.cuh"
}  // namespace nx

using namespace nx;

extern "C" {

int nx_trace_prev_access(nx_ctx* ctx, const nx_access_stream* streams, uint32_t n_streams, uint32_t n_key_cols, const uint32_t* key_bits,
                         uint32_t n_payload, const uint32_t* init, const nx_access_summary* summary, uint64_t* n_keys) {
    NX_GUARD(ctx);
    // the streams in the driver's shape: column streams, every rule GIVEN.  The driver refuses a NULL array and a count outside 1 .. 65536
    // before it reads a stream, so only a count it accepts is read here.
    const u32 n_read = streams && n_streams <= AH_MAX_STREAMS ? n_streams : 0;
    std::vector<nx_chain_stream> wide(n_read + 1);
    for (u32 i = 0; i < n_read; i++) {
        const nx_access_stream& s = streams[i];
        nx_chain_stream& w = wide[i]; memset(&w, 0, sizeof w);
        w.d_key = s.d_key; w.d_flag = s.d_flag; w.d_payload = s.d_payload; w.d_prev = s.d_prev; w.d_ordinal = s.d_ordinal;
        w.log_size = s.log_size; w.epoch = s.epoch; w.linear = s.linear;
    }
    return access_history<false>(ctx, "nx_trace_prev_access", streams ? wide.data() : nullptr, n_streams, n_key_cols, key_bits, n_payload, init, summary, n_keys);
}

}  // extern "C"
