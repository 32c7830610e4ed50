// Memory-checking columns for accesses that leave behind something that depends on what they found: nx_trace_access_chain.
//
// nx_trace_prev_access (prev_access.hip) resolves "what did the previous access to this address leave" when every access knows in
// advance what it leaves (load/store: last_access.insert(addr, (clk, value)), prover/src/chips/instructions/i/load_store.rs:199-205).
// The keccak chip does not: KeccakChip::update_state_timestamps (prover/src/chips/custom.rs:107-123) touches the 200 bytes at addr + i,
// reports the timestamp it finds and leaves ts + 1, so calls on one buffer chain through each other.  The kernels and the host driver
// are access_history.cuh's, in the instantiation with block streams, rules and chained columns; it is launched on every call, also on
// one that has no block stream and no ADD column.
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

int nx_trace_access_chain(nx_ctx* ctx, const nx_chain_stream* streams, uint32_t n_streams, uint32_t n_key_cols, const uint32_t* key_bits,
                          uint32_t n_payload, const uint32_t* init, const nx_access_summary* summary, uint64_t* n_keys) {
    NX_GUARD(ctx);
    return access_history<true>(ctx, "nx_trace_access_chain", streams, n_streams, n_key_cols, key_bits, n_payload, init, summary, n_keys);
}

}  // extern "C"
