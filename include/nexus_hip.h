/*
 * nexus_hip.h — C ABI of libnexus_hip.so, the MI355X (gfx950) backend for the Nexus zkVM
 * commit-and-prove hot path.
 *
 * The reference (nexus-xyz/nexus-zkvm) has no FFI today: it instantiates Stwo's CPU `SimdBackend`
 * directly (reference prover/src/machine.rs:16,186,203,286; prover2/machine/src/prove.rs:12,53,65,124).
 * The drop-in boundary is therefore the family of Stwo backend traits the reference relies on; each
 * entry point below names the trait method it replaces and the reference call site that reaches it.
 * A Rust `HipBackend` shim that binds these symbols is shown in INTEGRATION.md.
 *
 * Conventions
 *  - All field data are canonical M31 values in [0, 2^31-1), one uint32_t each, little endian.
 *    Secure-field (QM31) data are 4 coordinate words (a + bi) + (c + di)u  ->  {a, b, c, d};
 *    secure *columns* are 4 separate coordinate columns (Stwo `SecureColumnByCoords`).
 *  - Pointers named `d_*` / documented "device" are HIP device pointers (from nx_alloc, or any
 *    hipMalloc'd / torch-allocated memory on the context's device).  Pointer *arrays* such as
 *    `const uint32_t* const* cols` are HOST arrays holding device pointers.
 *  - ALIGNMENT.  A device column may lie at any 4-byte aligned address (a pointer into a slab, `ptr + k * len`, a row block), with these
 *    exceptions, whose kernels read and write 16 or 8 bytes at a time with no word path: a misaligned pointer is refused with NX_ERR_ARG
 *    before anything is launched — nx_last_error names the argument and the column index — and the context stays usable.
 *      16 bytes: the columns of nx_interpolate_batch (d_cols), nx_evaluate_batch (d_polys, d_out), nx_lde_batch / nx_lde_commit (d_cols,
 *      d_lde) and nx_commit_root (d_cols), nx_accumulate_quotients / nx_accumulate_quotients_partial (d_cols, d_out4); the node buffers
 *      of nx_merkle_commit_on_layer (d_prev_layer, d_out) and nx_merkle_leaf_chain (d_state_in, d_state_out).  The columns these two
 *      hash (d_cols) are read word by word and may lie anywhere.
 *      8 bytes: d_src4 of nx_fold_circle_into_line and nx_fold_line (a lane reads its pair as one word; the destinations are word
 *      accesses), the 64-bit side of nx_m31_widen (d_dst) and nx_m31_narrow (d_src).
 *    A column shorter than the access is exempt, it goes through a word kernel: transforms of 2 or 4 rows — nx_interpolate_batch below
 *    2^3 rows, the source of nx_evaluate_batch / nx_lde_batch / nx_commit_root below 2^2, an extension (d_out, d_lde) below 2^3 — and
 *    quotients of 2 rows.  So the 2-row columns nx_prover_tree_begin packs into one slab and the packed coordinates of 1- and 2-word
 *    secure columns are fine as they are.  nx_trace_keccak_round and nx_trace_keccak_memory_check state the same kind of rule for their
 *    d_states / d_states_out (8 bytes) and d_timestamps (16 bytes) themselves; their trace columns are written word by word.
 *    Entries whose host code chooses between a 16-byte and a word kernel by the pointers' low bits accept any word-aligned pointer and
 *    give the same words either way: nx_copy, nx_merkle_commit, nx_merkle_from_leaves, nx_upload_columns_narrow,
 *    nx_logup_multiplicities(_sparse), nx_trace_prev_access, nx_trace_program.  Every other entry touches caller memory word by word.
 *    tests/placement.py classifies every entry with the source lines; tests/test_gpu_placement.py runs each at every word offset.
 *  - Every function returns NX_OK (0) or a negative error code; nx_last_error() gives the text.
 *    Allocation failure is an error code, not a panic (reference: vec![] aborts, trace_builder.rs:29).
 *  - A context is single-threaded at the protocol level like the reference's prover
 *    (one &mut Blake2sChannel, machine.rs:197); all work is ordered on the context's HIP stream and
 *    is asynchronous; only functions that return data to the host synchronise.
 *  - Results are exact integers: bit-identical regardless of scheduling.
 */
#ifndef NEXUS_HIP_H
#define NEXUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NX_OK 0
#define NX_ERR_HIP (-1)       /* HIP runtime error (text in nx_last_error)                         */
#define NX_ERR_ARG (-2)       /* invalid argument                                                   */
#define NX_ERR_OOM (-3)       /* device or host allocation failed                                   */
#define NX_ERR_PROTOCOL (-4)  /* ProvingError::ConstraintsNotSatisfied / FRI invalid degree         */
#define NX_ERR_NO_DEVICE (-5) /* no gfx950 device visible — there is NO CPU fallback                */
#define NX_ERR_VERIFY (-6)    /* VerificationError: a well-formed proof failed a check of the verifier */

/* Merkle hash rule (unverifiable upstream detail kept switchable). */
#define NX_HASH_BLAKE2S 0      /* standard Blake2s-256 of (left ‖ right ‖ column values)            */
#define NX_HASH_BLAKE2S_RAW0 1 /* zero-state raw compression chaining, t = f = 0 (older Stwo)       */

/* FRI circle-column folding alpha. */
#define NX_FRI_ALPHA_PREV 0  /* fold circle columns with the previous layer's alpha (newer Stwo)    */
#define NX_FRI_ALPHA_FIRST 1 /* fold all circle columns with the first alpha (older Stwo)           */

/* Element kind of one host column of the narrow upload entry points (nx_upload_columns_narrow, nx_prover_tree_commit_host_narrow,
 * nx_prove_machine_host_narrow).  The device columns are u32 words whatever the kind. */
#define NX_COL_U32 0        /* uint32_t elements: what the u32 entry points take, handled exactly as they handle it         */
#define NX_COL_U16 1        /* uint16_t elements: sent as they are, widened on the device                                   */
#define NX_COL_U8 2         /* uint8_t elements: sent as they are, widened on the device                                    */
#define NX_COL_U32_AS_U16 3 /* uint32_t elements, every value < 2^16: packed to 2 bytes on host threads, sent narrow        */
#define NX_COL_U32_AS_U8 4  /* uint32_t elements, every value < 2^8: packed to 1 byte on host threads, sent narrow          */

typedef struct nx_ctx nx_ctx;
typedef struct nx_twiddles nx_twiddles;
typedef struct nx_tree nx_tree;

/* ---------------------------------------------------------------- context ------------------- */
int nx_ctx_create(int device, nx_ctx** out);
void nx_ctx_destroy(nx_ctx* ctx);
const char* nx_last_error(const nx_ctx* ctx); /* ctx may be NULL: last global error               */
int nx_ctx_set_hash_mode(nx_ctx* ctx, int mode);
/* Per-context policy and tuning.  The NX_* environment variables only seed a new context's defaults; what a
 * context does is decided by its own options, so two contexts of one process may differ.  Names: "fft.batch_cols" (2^22-row columns per launch of the LDE),
 * "fft.streams" (1..4), "comm.timeout_ms" (both library transports — native RCCL and the in-process one: the longest a rank waits for its peers in one collective before it
 * aborts the communicator / breaks the group and fails the prove, default 120000; 0 = wait for ever), "fri.dist_min_log", "dist.chunks" and "air.degree_split" (1: degree-aware composition, see
 * nx_air_constraint_degrees) — row-sharded prove: every GPU of a proof must use the same values of these three, they shape the
 * exchanges —, "air.segment" (instruction budget of one generated AIR kernel), "quotients.coeffs" (1: the DEEP quotients of a wide
 * size group are accumulated from the coefficient columns — half the bytes at blowup 2; one GPU only), "air.half_domain" (1: constraints
 * of degree <= 2 are evaluated on the first half of the committed 2N-point domain; one GPU, blowup 2), "air.quarter_domain" (constraints
 * of degree 4 are evaluated on the committed 2N rows plus the first quarter of the 4N-point domain — 3N + 1 samples instead of 4N;
 * a degree-5 quotient has 4N coefficients and is evaluated on all 4N points;
 * 1: only those that read no neighbour row, 2 (default): all of them, the columns read at a neighbour row — the reference's Pc /
 * IsPadding, prover/src/column.rs:13-20 — evaluated on the first HALF of that domain, which holds the neighbours of its first quarter;
 * one GPU, blowup 2, component bound 2).  Kernel-shape switches kept for A/B measurement (defaults are the
 * measured best): "fft.kmax" (most layers of a non-first FFT pass, 1..11), "fft.fused" (fused middle launch of the LDE), "merkle.subtree"
 * (highest level built by the fused sub-tree launch; 0 = one launch per level), "merkle.top" (the level, 1..10, from which ONE block
 * builds the rest of a tree), "merkle.pair_levels" (two node-only levels per launch
 * above it), "fri.device_channel", "fri.tail" (0 = off, 1 = the FRI layers of <= 2^11 points in one launch,
 * 2..11 = from 2^that many points), "logup.scan_tiled", "logup.per_column", "merkle.fused" (0..31, default 21; 0 = off, else the smallest log size from which a tree of <= 4 columns of one
 * size gets its leaf hash and 6 levels in one launch), "machine.logup_program" (default 0; 1: nx_prove_machine builds every wide-tuple component's interaction
 * trace through nx_logup_program), "machine.reuse_preprocessed" (default 0: every proof commits its preprocessed tree afresh, as the
 * reference does; 1: nx_prove_machine keeps the committed preprocessed tree of a statement shape in the context and adopts it in later
 * proofs of that shape — nx_prover_tree_adopt's rule; statements with a table component still fill theirs), "trace.vec4" (1, the default: nx_trace_program runs a program whose loads all have offset 0 with four
 * storage positions per lane — 16-byte loads and stores — instead of one row per lane).  "host.pack_threads" (1..64; default
 * min(16, hardware threads)): host threads that pack NX_COL_U32_AS_U16 / NX_COL_U32_AS_U8 columns of the narrow upload entry points.
 * Debug aids of the device block cache (default 0, NX_DEBUG_POISON / NX_DEBUG_POISON_FREE): "debug.poison" (1, 2, 3: every block the
 * context's allocator hands out — nx_alloc and every internal temporary, fresh or recycled — is filled whole with 0xA5A5A5A5, 0xFFFFFFFF
 * or 0x00000001 first, on the stream its owner's first write would take, with no synchronisation; the staging ring of pointer tables and
 * constants is filled when the option turns on and again where it wraps) and "debug.poison_free" (1, with "debug.poison" != 0: a block is
 * filled again when it goes back to the cache).  Code that reads a temporary before it wrote all of it, or frees a block something
 * still reads, then computes from the pattern instead of from zero pages or a previous call's values.
 * The device-memory budget of the context's block allocator (nx_alloc and every internal buffer): "mem.limit_bytes" (0 .. 2^62; 0, the
 * default, = none; NX_MEM_LIMIT_BYTES) bounds the bytes the context holds from the driver as blocks, live + cached.  A request of b bytes
 * (rounded up to 256) that no cached block of its size serves first gives the cache back to the driver when live + cached + b would pass
 * the limit; a request with live + b over the limit — cached block or not — is NX_ERR_OOM before any driver call, and nx_last_error names
 * the request, the live bytes and the limit ("dev_alloc: 16777216 bytes refused: 33554432 live of a budget of 41943040
 * (mem.limit_bytes)").  A limit below the current live count is accepted and refuses later requests only.  NOT blocks, and not counted:
 * the context's fixed buffers — the staging ring of pointer tables and constants (16 MiB of device memory and its 16 MiB pinned host
 * mirror, from nx_ctx_create on), the bounce buffer of the blocking copies (2 x 4 MiB pinned host memory, from the first copy of >= 32 KiB
 * on) and the pack ring of the narrow upload (pinned host memory, two slots of 16 columns x 2^log_size rows x 2 bytes, from the first
 * packed column until nx_ctx_trim).  "mem.cache_bytes" (0 .. 2^62; default 192 GiB, NX_MEM_CACHE_BYTES): the most bytes of freed blocks
 * kept for reuse; a free that takes the cache beyond it hands the whole cache back to the driver, which synchronises the context as
 * nx_ctx_trim does; 0 = every freed block goes back at once.  "mem.cached_bytes" (read-only): the bytes of freed blocks held now.
 * "debug.fail_alloc" (n >= 1; default 0): the n-th request the allocator sees from now on is refused once with NX_ERR_OOM ("debug.fail_alloc:
 * request n (B bytes) refused"), decided on the host before any driver call, and the option is 0 again; "debug.alloc_count" (read-only:
 * setting it is NX_ERR_ARG) is the number of requests the allocator has seen since nx_ctx_create — the difference around a call is the
 * number of positions a sweep of that call has to visit.
 *
 * AFTER NX_ERR_OOM — the rule of every entry of this header that takes a context or a handle made from one, whatever refused the
 * request (the driver, "mem.limit_bytes", "debug.fail_alloc"): (1) nx_ctx_memory's live count is what it was before the call: every
 * block the call took has gone back to the cache, in the order the success path returns them; (2) every *out handle is NULL: no
 * nx_tree, nx_twiddles, nx_trace_partition, nx_air_kernel, nx_prover or shared tree is left half-made, and output columns of the caller hold
 * unspecified words; (3) a session (nx_prover) is in the state documented for the refused narrow upload: the transcript is untouched, a
 * begun tree is no longer begun and may be begun again, a failed nx_prover_prove has restored the channel; (4) the context stays usable:
 * the same call repeated returns the words it always returns; (5) a row-sharded prove aborts its transport (nx_comm.abort) so that no
 * peer waits out "comm.timeout_ms": after nx_comm_group_reset (or a new communicator) the group proves again.
 * Unknown names and out-of-range values are NX_ERR_ARG.
 * None of them changes a result: proofs, roots and transforms are bit-identical under every setting. */
int nx_ctx_set_option(nx_ctx* ctx, const char* name, int64_t value);
int nx_ctx_get_option(const nx_ctx* ctx, const char* name, int64_t* value);
int nx_sync(nx_ctx* ctx);
/* Hands the context's cached device blocks (freed columns kept for the next prove of the same shape) back to the driver:
 * another context, process or library on the same GPU can then use that memory.  Synchronises the context. */
int nx_ctx_trim(nx_ctx* ctx);
void* nx_ctx_stream(nx_ctx* ctx); /* hipStream_t the context launches on                       */
/* The context allocator's own count: bytes of device memory it has handed out and not taken back (nx_alloc and every internal buffer;
 * cached free blocks are not counted), and the high-water mark of that count since the last reset (reset_peak != 0: the mark restarts
 * at the current count).  Either pointer may be NULL.  Host only.  How nx_commit_root's memory bound is checked. */
int nx_ctx_memory(nx_ctx* ctx, uint64_t* live_bytes, uint64_t* peak_bytes, int reset_peak);
const char* nx_version(void);

/* ------------------------------------------- columns: Column / ColumnOps ------------------- */
/* Column::zeros / from_iter / to_cpu (reference prover2/trace/src/builder.rs:103,
 * prover2/trace/src/component.rs:40-44; BaseColumn in prover/src/trace/utils.rs:100). */
int nx_alloc(nx_ctx* ctx, size_t n_words, uint32_t** d_out);
int nx_free(nx_ctx* ctx, uint32_t* d_ptr);
int nx_memset_zero(nx_ctx* ctx, uint32_t* d_ptr, size_t n_words);
int nx_upload(nx_ctx* ctx, uint32_t* d_dst, const uint32_t* h_src, size_t n_words);
int nx_download(nx_ctx* ctx, uint32_t* h_dst, const uint32_t* d_src, size_t n_words);
/* Column::clone on device (the reference clones whole traces before committing them: prover/src/machine.rs:210-214,232;
 * prover2/trace/src/component.rs:75).  Stream-ordered; src and dst must not overlap.  Any word-aligned pointers and any length: 16-byte
 * copies when both pointers are 16-byte aligned and n_words is a multiple of 4, a plain device copy otherwise. */
int nx_copy(nx_ctx* ctx, uint32_t* d_dst, const uint32_t* d_src, size_t n_words);
/* Gather scattered words: out[i] = d_ptrs[i][index[i]] (decommitment reads, MerkleProver::decommit). */
int nx_gather(nx_ctx* ctx, const uint32_t* const* d_ptrs, const uint64_t* index, size_t n, uint32_t* h_out);

/* K1 — ColumnOps<M31>::bit_reverse_column (reference prover/src/trace/utils.rs:101,
 * prover2/trace/src/utils.rs:109).  In place. */
int nx_bit_reverse(nx_ctx* ctx, uint32_t* d_col, uint32_t log_size);

/* R3 — finalize_columns fused on device (reference prover/src/trace/utils.rs:94-106 +
 * prover/src/trace/utils_external.rs:24-39): natural coset order -> bit-reversed circle-domain
 * order, n_cols columns of 2^log_size words; src and dst must not alias. */
int nx_finalize_columns(nx_ctx* ctx, const uint32_t* const* d_src_natural, uint32_t* const* d_dst,
                        uint32_t n_cols, uint32_t log_size);
/* Same, source on the host (the trace the AIR layer filled, TracesBuilder cols, trace_builder.rs:19-32). */
int nx_upload_coset_order(nx_ctx* ctx, const uint32_t* h_natural, uint32_t log_size, uint32_t* d_dst);
/* The same for a whole host-resident trace: every host column is pinned in place, streamed over
 * PCIe on a side stream and permuted on device behind the copy (coset_order != 0) or stored as is (the host already holds
 * bit-reversed circle-domain order).  Blocking: the host columns are free on return.  Replaces the per-column CPU passes of
 * finalize_columns + into_circle_evaluation's clones (reference prover/src/trace/utils.rs:94-106, trace_builder.rs:156-164). */
int nx_upload_columns(nx_ctx* ctx, const uint32_t* const* h_cols, uint32_t n_cols, uint32_t log_size,
                      uint32_t* const* d_cols, int coset_order);
/* A trace buffer that is reused from proof to proof is pinned ONCE by its owner instead of once per upload: nx_host_pin registers
 * [h, h + bytes) with the driver (hipHostRegister; the memory stays where it is), nx_host_unpin releases it.  Every entry point that takes
 * host columns (nx_upload_columns, nx_prover_tree_commit_host, nx_prove_machine_host) recognises pinned columns and skips its own
 * pin / unpin of them — the per-proof cost of pinning 6 GB of trace is what separates 135 ms from the PCIe floor in bench.py's
 * host_trace block.  Pinning is an optimisation only: results never depend on it.  Pinned ranges must not overlap (NX_ERR_ARG; the
 * book is process-wide, any context recognises them); nx_host_unpin takes the start of a pinned range and waits for the calling
 * context's copies out of it. */
int nx_host_pin(nx_ctx* ctx, const void* h, size_t bytes);
int nx_host_unpin(nx_ctx* ctx, const void* h);
/* nx_upload_columns for a trace whose columns are byte or half-word limbs: nearly every main column of the reference is a byte limb stored
 * as u32 (IntoBaseFields for u32, prover/src/trace/utils.rs:57-61, filled by TracesBuilder, trace_builder.rs:19-32), so the u32 form
 * sends four bytes per byte over PCIe.  kinds[i] (NX_COL_*; NULL = all NX_COL_U32) says what h_cols[i] holds.  NX_COL_U16 / NX_COL_U8
 * columns are pinned in place at their real byte length (2^log_size x 2 or 1 bytes; a range pinned with nx_host_pin is recognised by
 * that length) or go through the bounce buffer when they cannot be pinned, are copied as they are and widened on the device — fused
 * with R3's permutation when coset_order != 0.  NX_COL_U32_AS_U16 / NX_COL_U32_AS_U8 columns are never pinned: "host.pack_threads"
 * threads pack them into a pinned staging ring of the context (allocated on first use, released by nx_ctx_trim / nx_ctx_destroy) while
 * the previous chunk of 16 columns is on the bus.  A value that does not fit its declared width is refused, never truncated: NX_ERR_ARG,
 * and nx_last_error names the kind, the value, the column (index into h_cols) and the row (index into that column) — the lowest
 * column, then row, whatever the thread count; the chunk that holds it is never sent, the caller's arrays are never written and the
 * context stays usable.  A call whose columns are all NX_COL_U32 is nx_upload_columns.  Blocking: the host columns are free on return.
 * NX_ERR_ARG for NULL arguments, zero columns or an unknown kind.  d_cols: any word-aligned pointers (a column that is not 16-byte aligned
 * is widened one value per lane). */
int nx_upload_columns_narrow(nx_ctx* ctx, const void* const* h_cols, const uint8_t* kinds, uint32_t n_cols, uint32_t log_size,
                             uint32_t* const* d_cols, int coset_order);

/* ----------------------------------------------------- K2-K4, K7: PolyOps ------------------ */
/* K2 — PolyOps::precompute_twiddles(CanonicCoset::new(log_half_coset + 1).half_coset())
 * (reference prover/src/machine.rs:186-194, prover2/machine/src/prove.rs:53-57, verify.rs:121). */
int nx_twiddles_create(nx_ctx* ctx, uint32_t log_half_coset, nx_twiddles** out);
void nx_twiddles_destroy(nx_twiddles* tw);
/* Test/debug access: copies the 2^log_half_coset forward and inverse twiddles to the host. */
int nx_twiddles_download(nx_ctx* ctx, const nx_twiddles* tw, uint32_t* h_tw, uint32_t* h_itw);

/* K3 — PolyOps::interpolate_columns via TreeBuilder::extend_evals (reference
 * prover/src/machine.rs:209,226,232,235,250,260).  In place: bit-reversed evaluations on
 * CanonicCoset(log_size).circle_domain() -> coefficients. */
int nx_interpolate_batch(nx_ctx* ctx, const nx_twiddles* tw, uint32_t* const* d_cols, uint32_t n_cols,
                         uint32_t log_size);
/* K4 — PolyOps::evaluate_polynomials via TreeBuilder::commit -> CommitmentTreeProver::new
 * (reference prover/src/machine.rs:228,237,263).  Coefficients (2^log_size) -> bit-reversed
 * evaluations on CanonicCoset(log_size + log_expand).circle_domain(); out-of-place. */
int nx_evaluate_batch(nx_ctx* ctx, const nx_twiddles* tw, const uint32_t* const* d_polys, uint32_t n_cols,
                      uint32_t log_size, uint32_t log_expand, uint32_t* const* d_out);
/* K3+K4 fused — what TreeBuilder::extend_evals followed by TreeBuilder::commit computes for one group of
 * equally sized columns (reference prover/src/machine.rs:232-237): d_cols holds bit-reversed evaluations on
 * entry and the coefficients on return; d_lde receives the evaluations on the blown-up domain.  Each column
 * batch runs iFFT and FFT back to back so the coefficients stay on chip between the two transforms. */
int nx_lde_batch(nx_ctx* ctx, const nx_twiddles* tw, uint32_t* const* d_cols, uint32_t n_cols, uint32_t log_size,
                 uint32_t log_blowup, uint32_t* const* d_lde);
/* K7 — PolyOps::eval_at_point (inside stwo::prover::prove, reference machine.rs:286):
 * out[i] = polys[poly_idx[i]] evaluated at points[i] (8 words x‖y each), all polys of one log_size. */
int nx_eval_at_points(nx_ctx* ctx, const uint32_t* const* d_polys, uint32_t log_size, const uint32_t* poly_idx,
                      const uint32_t* h_points, uint32_t n_evals, uint32_t* h_out /* 4 words each */);

/* ------------------------------------------- K5/K6: MerkleOps<Blake2sMerkleHasher> --------- */
/* MerkleProver::commit -> MerkleOps::commit_on_layer per layer (reference machine.rs:228,237,263).
 * Columns in commit order (stable-sorted by size inside); log_sizes are the column (LDE) sizes.  Any word-aligned column pointers: the
 * fused launch ("merkle.fused") is taken only when every column is 16-byte aligned, the per-level kernels read words. */
int nx_merkle_commit(nx_ctx* ctx, const uint32_t* const* d_cols, const uint32_t* log_sizes, uint32_t n_cols,
                     nx_tree** out);
int nx_merkle_root(nx_ctx* ctx, const nx_tree* tree, uint8_t root[32]); /* roots(): machine.rs:411 */
uint32_t nx_merkle_n_layers(const nx_tree* tree);
/* Device pointer of layer k (2^k nodes x 8 words); layer 0 is the root. */
const uint32_t* nx_merkle_layer(const nx_tree* tree, uint32_t k);
void nx_tree_destroy(nx_tree* tree);

/* MerkleOps<Blake2sMerkleHasher>::commit_on_layer itself — ONE layer: node i = H(prev[2i] ‖ prev[2i+1] ‖ cols[0][i] ‖ cols[1][i] ...);
 * d_prev_layer: the 2^(log_size+1) nodes of the layer below (8 words each) or NULL for the leaf layer; d_cols: the columns of
 * 2^log_size words injected at this layer (commit order); d_out: 2^log_size nodes.  Hash rule = nx_ctx_set_hash_mode.
 * (MerkleProver::commit, the loop over layers, is nx_merkle_commit.) */
int nx_merkle_commit_on_layer(nx_ctx* ctx, uint32_t log_size, const uint32_t* d_prev_layer, const uint32_t* const* d_cols, uint32_t n_cols,
                              uint32_t* d_out);
/* MerkleProver::decommit(queries_per_log_size, columns) (inside stwo::prover::prove, reference machine.rs:286-290): the values of
 * `columns` (commit order, LDE log sizes) at the queried rows and the MerkleDecommitment {hash_witness, column_witness}.
 * One (query_logs[i], query_counts[i]) pair per queried layer; `queries` holds every layer's sorted, distinct positions back to
 * back.  Outputs are malloc'd (nx_free_host); hash_witness: 8 words per hash. */
int nx_merkle_decommit(nx_ctx* ctx, const nx_tree* tree, const uint32_t* const* d_cols, const uint32_t* log_sizes, uint32_t n_cols,
                       const uint32_t* query_logs, const uint32_t* query_counts, uint32_t n_query_logs, const uint64_t* queries,
                       uint32_t** queried_values, size_t* n_queried_values, uint32_t** hash_witness, size_t* n_hashes,
                       uint32_t** column_witness, size_t* n_column_witness);

/* Column-sharded commitment (BASELINE config #4).  A tree leaf is one sequential Blake2s chain
 * over ALL columns of the tree (16 columns = one 64-byte block), so column shards of one tree are chained:
 * the GPU that owns columns [col_offset, col_offset + n_cols) of a layer with total_cols columns continues the
 * 8-word chaining state of rows [row_begin, row_begin + n_rows) received from the previous GPU (d_state_in == NULL
 * for the shard that starts at column 0) and hands its state on; col_offset must be a multiple of 16.  The shard
 * that holds the last column applies the hash finalisation, so its d_state_out rows are the leaf digests.
 * d_state_in / d_state_out: n_rows x 8 words, indexed by row - row_begin (may alias).  d_cols: full columns
 * of 2^log_size words. */
int nx_merkle_leaf_chain(nx_ctx* ctx, const uint32_t* const* d_cols, uint32_t n_cols, uint32_t log_size,
                         uint32_t col_offset, uint32_t total_cols, const uint32_t* d_state_in, uint32_t* d_state_out,
                         uint64_t row_begin, uint64_t n_rows);
/* MerkleProver over already hashed leaves: builds the inner layers above 2^log_size leaf digests (8 words each,
 * copied in, nx_copy's rule: any word-aligned pointer) — the part of a sharded commit the last GPU of the chain runs before broadcasting
 * the root. */
int nx_merkle_from_leaves(nx_ctx* ctx, const uint32_t* d_leaf_digests, uint32_t log_size, nx_tree** out);

/* ------------------------------------------------------------- K8: QuotientOps ------------- */
/* QuotientOps::accumulate_quotients (inside prove).  One size group: n_cols columns of
 * 2^log_size words; sample batches flattened: batch b has batch_counts[b] (column, value) pairs,
 * column indices in col_idx, sampled values (4 words each) in values, point (8 words) in points.
 * random_coeff is the DEEP alpha (4 words).  d_out4: 4 coordinate columns of 2^log_size words. */
int nx_accumulate_quotients(nx_ctx* ctx, uint32_t log_size, const uint32_t* const* d_cols, uint32_t n_cols,
                            const uint32_t random_coeff[4], uint32_t n_batches, const uint32_t* points,
                            const uint32_t* batch_counts, const uint32_t* col_idx, const uint32_t* values,
                            uint32_t* const* d_out4);

/* Column-sharded variant: the quotient is a sum over columns, so each GPU accumulates the entries whose
 * columns it holds (entry_local[k] != 0; col_idx[k] then indexes ITS d_cols) with the alpha power of the entry's GLOBAL
 * position, exactly one GPU adds the line terms of all entries (include_line_terms), and the partial results are summed
 * mod p across GPUs (nx_comm.allreduce_m31).  Batches, counts, values describe ALL entries, on every GPU.  col_idx of a non-local
 * entry (entry_local[k] == 0) is ignored, whatever it holds (0xFFFFFFFF by convention); entry_local == NULL means every entry is
 * local, and with include_line_terms the call is then nx_accumulate_quotients.  n_cols == 0 is allowed (a GPU that holds no column of
 * this size group; d_cols may then be NULL): it still passes every entry, and writes the line terms or, without them, zeros. */
int nx_accumulate_quotients_partial(nx_ctx* ctx, uint32_t log_size, const uint32_t* const* d_cols, uint32_t n_cols,
                                    const uint32_t random_coeff[4], uint32_t n_batches, const uint32_t* points,
                                    const uint32_t* batch_counts, const uint32_t* col_idx, const uint32_t* values,
                                    const uint8_t* entry_local, int include_line_terms, uint32_t* const* d_out4);

/* --------------------------------------------------------------- K9: FriOps ---------------- */
/* FriOps::fold_circle_into_line: dst (line evaluation, 2^(src_log-1)) = dst*alpha^2 + fold(src). */
int nx_fold_circle_into_line(nx_ctx* ctx, const nx_twiddles* tw, uint32_t* const* d_dst4,
                             const uint32_t* const* d_src4, uint32_t src_log, const uint32_t alpha[4]);
/* FriOps::fold_line: src on the line domain half_odds(src_log + n_doublings) doubled n_doublings
 * times (log size src_log) -> dst of log size src_log - 1. */
int nx_fold_line(nx_ctx* ctx, const nx_twiddles* tw, const uint32_t* const* d_src4, uint32_t src_log,
                 uint32_t n_doublings, const uint32_t alpha[4], uint32_t* const* d_dst4);

/* ------------------------------------------- the rest of the Backend supertraits -------------------
 * Called by stwo::prover::prove through `B: Backend` (reference machine.rs:286-290, prove.rs:124-128); not hot spots here (the
 * composition accumulator and the logup kernels fuse what they need) but required for a per-op HipBackend to type-check. */
/* AccumulationOps::accumulate: dst[k][i] += src[k][i] on 4 coordinate columns of 2^log_size words. */
int nx_secure_accumulate(nx_ctx* ctx, uint32_t* const* d_dst4, const uint32_t* const* d_src4, uint32_t log_size);
/* AccumulationOps::generate_secure_powers: out = [1, felt, felt^2, ...] (host; 4 words each). */
int nx_generate_secure_powers(const uint32_t felt[4], uint32_t n_powers, uint32_t* out);
/* FieldOps<BaseField>::batch_inverse / FieldOps<SecureField>::batch_inverse: element-wise inverses (inputs must be non-zero,
 * as Stwo requires); src and dst may alias. */
int nx_batch_inverse_m31(nx_ctx* ctx, const uint32_t* d_src, uint32_t* d_dst, size_t n);
int nx_batch_inverse_qm31(nx_ctx* ctx, const uint32_t* const* d_src4, uint32_t* const* d_dst4, size_t n);
/* ColumnOps<SecureField>::bit_reverse_column (a SecureColumnByCoords is 4 base columns). */
int nx_bit_reverse_secure(nx_ctx* ctx, uint32_t* const* d_col4, uint32_t log_size);
/* FriOps::decompose(eval) -> (g, lambda): lambda = (sum of the first half - sum of the second half) / 2^log_size of the
 * bit-reversed circle evaluation, g = eval -/+ lambda on the first / second half [upstream-recollection; not called by
 * FriProver::commit at the pinned revision as far as the reference's use of it shows — exported for trait completeness]. */
int nx_fri_decompose(nx_ctx* ctx, const uint32_t* const* d_src4, uint32_t log_size, uint32_t* const* d_g4, uint32_t lambda[4]);

/* --------------------------------------------------------------- K10: GrindOps ------------- */
/* GrindOps<Blake2sChannel>::grind: smallest nonce with >= pow_bits trailing zero bits of
 * Blake2s(digest ‖ nonce_le64) read as a little-endian u128.  The search runs in launches of at most 2^24 nonces, the first one 64 x
 * 2^pow_bits of them: from about 22 bits the smallest nonce often lies beyond the first launch and the search takes several. */
int nx_grind(nx_ctx* ctx, const uint8_t digest[32], uint32_t pow_bits, uint64_t* nonce);

/* ------------------------------------------- synthetic machine (BASELINE configs #2-#4) ---- */
/* The reference's AIR closures (MachineEval::evaluate, prover/src/components/mod.rs:48-56) are
 * generic Rust and cannot cross a C ABI (last row).  For measurement the library
 * carries the synthetic wide-Fibonacci-style machine of SURVEY.md §8(d): */
typedef struct nx_component_spec {
    uint32_t log_size, n_pre, n_main, n_inter;
    /* The component's log constraint-degree bound: its constraints are evaluated on CanonicCoset(log_size + bound) and the composition
     * polynomial has log size max over components of (log_size + bound) — per component as in the reference (v1: the main component
     * +2, prover/src/components/mod.rs:12,44-45, every extension +1, prover/src/extensions/multiplicity.rs:108-110; prover2: 1, the
     * shifts 2, prover2/machine/src/framework/traits/builtin.rs:23, composition size = the maximum, prove.rs:44-48).
     * 0 = nx_pcs_config.log_constraint_degree; otherwise 1 <= bound <= that field (the twiddle tree is sized by the config's). */
    uint32_t log_constraint_degree_bound;
    /* nx_prove_machine only — how the component's F logup fractions fill its L = n_inter / 4 logup columns (NX_LOGUP_* below). */
    uint32_t logup_mode;
} nx_component_spec;
/* nx_component_spec.logup_mode, a bit set:
 *   0                 one fraction per column, F = L: EvalAtRow::finalize_logup as the v1 main component and the multiplicity tables
 *                     use it (reference prover/src/components/mod.rs:53, prover/src/extensions/multiplicity.rs:123) — degree-2 constraints;
 *   NX_LOGUP_PAIRS    two fractions per column, F = 2 L: finalize_logup_in_pairs (reference prover/src/extensions/keccak/round/
 *                     constraints.rs:116, keccak/memory_check/constraints.rs:125, extensions/final_reg.rs:112, every prover2 component:
 *                     prover2/machine/src/components/.../mod.rs) over columns built pairwise, (a d + b c) / (b d), by
 *                     LogupTraceBuilder::add_to_relation_with (prover2/machine/src/lookups/logup_trace_builder.rs:86-101) — the
 *                     constraint (S_j - S_{j-1}) d0 d1 - (n0 d1 + n1 d0) has degree 3 under the bound +1;
 *   NX_LOGUP_ODD      with PAIRS: F = 2 L - 1, the last column holds the one left-over fraction (LogupTraceBuilder::finalize,
 *                     logup_trace_builder.rs:110-117; finalize_logup_in_pairs with an odd number of add_to_relation calls);
 *   NX_LOGUP_TABLE    the table side of a lookup: every tuple reads PREPROCESSED columns (get_preprocessed_column) and every numerator is
 *                     a negated multiplicity column of the main trace (reference prover/src/extensions/multiplicity.rs:111-124,
 *                     extensions/keccak/bitwise_table/mod.rs). */
enum { NX_LOGUP_PAIRS = 1, NX_LOGUP_ODD = 2, NX_LOGUP_TABLE = 4 };
/* Bits 4..7 of logup_mode: the TUPLE SCHEDULE — how wide the relation tuples of the component's fractions are and what their entries are.
 *   0                 one- / two-column tuples (rounds 2-5);
 *   NX_TUPLES_V1      v1's chips: widths cycling 1, 1, 4, 1, 9, 1, 3, 1 — range checks (reference prover/src/chips/range_check/range256.rs:37),
 *                     [op_type CONSTANT, b, c, a] with a flag COLUMN as numerator (chips/instructions/i/bit_op.rs:31,341-365), register memory
 *                     (memory_check/register_mem_check.rs:34), and a 3-wide entry list holding a constant and a SUM of two columns;
 *   NX_TUPLES_KECCAK  3- / 4-wide bitwise lookups (chips/custom.rs:33-37) and, as the component's last two fractions, the 200-wide state
 *                     lookups with the numerators (is_padding - 1) and (1 - is_padding) (chips/custom.rs:45-46,
 *                     extensions/keccak/round/constraints.rs:101-110): expression numerators — their interaction trace comes from the
 *                     recorded relation entries (nx_logup_program);
 *   NX_TUPLES_V2      prover2's relations: 9, 21, 14, 10, 4, 12, 8 wide (prover2/machine/src/lookups/relations.rs:33-90).
 * The context option "machine.logup_program" = 1 sends every wide-tuple component through nx_logup_program (same bytes). */
#define NX_LOGUP_TUPLES(k) ((uint32_t)(k) << 4)
enum { NX_TUPLES_V1 = 1, NX_TUPLES_KECCAK = 2, NX_TUPLES_V2 = 3 };

typedef struct nx_pcs_config {
    uint32_t pow_bits, log_blowup, n_queries, log_last_layer_degree_bound; /* PcsConfig / FriConfig */
    uint32_t hash_mode, fri_alpha_mode;                                    /* switchable rules       */
    uint32_t log_constraint_degree;   /* 1 or 2 (components/mod.rs:12): the default AND the largest per-component bound (twiddle sizing, machine.rs:184-194) */
} nx_pcs_config;

typedef struct nx_prove_stats { /* milliseconds, device-synchronised stage boundaries */
    double trace_gen, commit, composition, oods, quotients, fri, pow, decommit, total;
    double lde_kernel_ms;        /* sum of Circle-FFT kernel time inside commits (HIP events)   */
    uint64_t lde_algorithmic_bytes;
    double merkle_kernel_ms;
    uint64_t merkle_algorithmic_bytes;
    double interaction;          /* logup interaction-trace generation (nx_prove_machine)         */
    double comm_ms;              /* wall time inside nx_comm callbacks (one proof on several GPUs) */
    uint64_t comm_bytes;         /* bytes this GPU sent to its peers                               */
    /* collectives this GPU entered during the prove, by kind — each is also a host synchronisation of the stream (one proof on several
     * GPUs): all-to-all of column shards into row blocks, all-gathers of device buffers, all-gathers of host words (roots, sampled
     * values, votes).  DESIGN.md section 7 bounds them by the statement's shape; tests/test_gpu_machine.py holds the bound. */
    uint32_t n_alltoallv, n_allgather_dev, n_allgather_host, n_comm_reserved;
} nx_prove_stats;

/* Fill tree `tree` (0 preprocessed / 1 main / 2 interaction) of the synthetic trace directly in
 * bit-reversed circle-domain order: d_cols holds, component after component, n_* columns. */
int nx_synth_fill_tree(nx_ctx* ctx, const nx_component_spec* comps, uint32_t n_comps, uint32_t tree,
                       uint64_t seed, uint64_t inter_seed, uint32_t* const* d_cols);

/* Full prove of the synthetic machine: the orchestration of reference prover/src/machine.rs:184-296
 * and stwo::prover::prove on device.  Returns a malloc'd proof in the flat "NXP1" u32 wire format
 * (free with nx_free_host). stats may be NULL.
 * SIZES.  The argument check admits 1 <= log_size <= 28, but a statement PROVES only if its smallest component has
 * log_size >= log_last_layer_degree_bound + 2 — with the default bound of 0: at least four rows.  Below that the component's
 * quotient column is no larger than FRI's last layer and never folds into a line: the prove runs up to the FRI commit phase and then
 * returns NX_ERR_PROTOCOL ("fri: first-layer columns not consumed"), as Stwo's FriProver does; nothing stays allocated and the context
 * remains usable.  The same holds for nx_prove_machine, nx_prove_machine_host and nx_prover_prove. */
int nx_prove_synth(nx_ctx* ctx, const nx_component_spec* comps, uint32_t n_comps, const nx_pcs_config* cfg,
                   uint64_t seed, const uint8_t* ad, size_t ad_len, uint32_t** proof_words, size_t* n_words,
                   nx_prove_stats* stats);
void nx_free_host(void* p);

/* EXPERIMENTAL until a real postcard dump of the reference has been replayed (tools/dump_reference.rs -> tools/replay_reference_dump.py):
 * the field order below is a recollection of Stwo @ 0790eba's derive(Serialize) declarations; a wrong order yields unparseable bytes.
 * The reference's proof bytes: `nexus_vm_prover::machine::Proof { stark_proof, claimed_sum, log_size }` (reference
 * prover/src/machine.rs:93-98) in postcard, the serde format the SDK ships proofs in (reference sdk/Cargo.toml:22,
 * sdk/src/stwo/seq.rs:60-64), from an NXP1 word stream plus the per-component claimed sums (4 words each) and log sizes.  Field
 * order = Stwo's derive(Serialize) declarations [upstream-recollection — pinned only once tools/dump_reference.rs has run on a box
 * with cargo].  Host arithmetic only (no context).  *bytes: free with nx_free_host. */
int nx_proof_serialize_stwo(const uint32_t* proof_words, size_t n_words, const uint32_t* claimed_sums, const uint32_t* log_sizes,
                            uint32_t n_components, uint8_t** bytes, size_t* n_bytes);

/* The reference-shaped machine: as nx_prove_synth, but the interaction tree is a REAL logup trace — lookup elements (z, alpha) drawn
 * after the main commit (reference machine.rs:239-240), one fraction per logup column over main-trace columns
 * (LogupTraceGenerator, reference traits.rs:124-145, chips/range_check/range256.rs:271-288: nx_logup_col per column, then
 * nx_logup_finalize_last), claimed sums mixed before the commit (machine.rs:262) — and the AIR (transition, degree-2 and logup
 * constraints with the [-1, 0] mask of the last logup column) is a recorded program compiled by nx_air_compile: the route a Rust
 * shim takes for the reference's own AIR.  n_inter = 4 x (logup columns of the component).  comm: NULL = one GPU; otherwise ONE
 * proof on the GPUs of the communicator (nx_comm below). */
struct nx_comm;
/* The HIP source nx_air_compile generates for the recorded AIR of one such component (host only; free with nx_free_host). */
int nx_machine_air_source(const nx_component_spec* comp, char** h_source);
/* The recorded program itself (host only): what nx_prove_machine hands to nx_air_compile for this component under a configuration
 * whose log_constraint_degree is cfg_log_constraint_degree — so that a CPU checker can run the product's emission through its own
 * interpreter.  Secure constants: [z, alpha, claimed / N, 0].  *h_program: free with nx_free_host. */
struct nx_cinstr;
int nx_machine_air_program(const nx_component_spec* comp, uint32_t cfg_log_constraint_degree, struct nx_cinstr** h_program,
                           uint32_t* n_instr, uint32_t* n_regs, uint32_t* n_constraints);
int nx_prove_machine(nx_ctx* ctx, const nx_component_spec* comps, uint32_t n_comps, const nx_pcs_config* cfg, uint64_t seed,
                     const uint8_t* ad, size_t ad_len, const struct nx_comm* comm, uint32_t** proof_words, size_t* n_words,
                     nx_prove_stats* stats);
/* The same machine with its preprocessed and main traces handed over in HOST memory — the hand-over of the reference, whose trace builder
 * fills `Vec<Vec<M31>>` on the CPU (prover/src/trace/trace_builder.rs:19-32) — instead of generated on the device: h_pre_cols / h_main_cols
 * hold, component after component, the n_pre / n_main columns of 2^log_size words (natural coset order when coset_order != 0, else
 * bit-reversed circle-domain order).  The two commits upload the columns in chunks and transform each chunk as it arrives
 * (nx_prover_tree_commit_host describes the pipeline); the interaction trace is generated on the device as in nx_prove_machine.  One GPU.
 * The proof equals nx_prove_machine's for the same trace, byte for byte.  This is what bench.py's `host_trace` block times. */
int nx_prove_machine_host(nx_ctx* ctx, const nx_component_spec* comps, uint32_t n_comps, const nx_pcs_config* cfg,
                          const uint32_t* const* h_pre_cols, const uint32_t* const* h_main_cols, int coset_order, const uint8_t* ad,
                          size_t ad_len, uint32_t** proof_words, size_t* n_words, nx_prove_stats* stats);
/* nx_prove_machine_host with an element kind per host column (NX_COL_*; nx_upload_columns_narrow describes the kinds, the pinning and
 * the refusal): pre_kinds[i] / main_kinds[i] for h_pre_cols[i] / h_main_cols[i], NULL = all NX_COL_U32.  The byte limbs of the
 * reference's main trace (trace_builder.rs:19-32) cross PCIe as bytes.  A refused value fails the proof with NX_ERR_ARG naming the
 * trace (preprocessed / main), the column index within that array and the row; nothing of the proof is returned and the context can
 * prove again.  One GPU; blocking; the host columns are free on return.  The proof equals nx_prove_machine_host's for the same values. */
int nx_prove_machine_host_narrow(nx_ctx* ctx, const nx_component_spec* comps, uint32_t n_comps, const nx_pcs_config* cfg,
                                 const void* const* h_pre_cols, const uint8_t* pre_kinds, const void* const* h_main_cols,
                                 const uint8_t* main_kinds, int coset_order, const uint8_t* ad, size_t ad_len, uint32_t** proof_words,
                                 size_t* n_words, nx_prove_stats* stats);
/* `Proof.claimed_sum` of the last successful nx_prove_machine on this context (reference prover/src/machine.rs:93-98: the proof the
 * reference returns carries the per-component logup claimed sums next to the StarkProof; a verifier mixes them before the interaction
 * commitment, machine.rs:262 / :448-450, and nx_proof_serialize_stwo takes them): 4 words per component, in component order.
 * Writes min(cap_components, n) entries and the count n.  Host only (no device work). */
int nx_machine_claimed_sums(const nx_ctx* ctx, uint32_t* claimed_sums, uint32_t cap_components, uint32_t* n_components);

/* ------------------------------------------- ONE proof on the GPUs of a node (BASELINE configs #4 / #5) ---------------
 * One process (or thread) per GPU calls the prove entry with the same arguments and its own nx_comm; W must be a power of two.
 * The LDE is column-parallel: every GPU transforms a contiguous share of each tree's columns.  One all-to-all per tree then turns
 * column shards into ROW BLOCKS — GPU r holds rows [r M/W, (r+1) M/W) of every LDE column (a contiguous block of the bit-reversed
 * domain = a subtree of the Merkle tree), so leaf hashing, constraint evaluation, DEEP quotients and the first FRI folds are
 * local.  Besides the transposition only these cross the links: the W subtree roots of every tree (all-gather, 32 B each), the
 * sampled and queried values (KBs), the columns read at a non-zero mask offset, the composition accumulator (all-gather of 4
 * columns) and the small FRI tail.  Every GPU returns the same proof, bit-identical to the single-GPU proof.
 * The transport is the caller's: RCCL over xGMI (nexus-zkvm_amd/sharded.py wraps torch.distributed) or anything else.  Device
 * buffers handed to a callback are complete when it is called and must be complete when it returns.  Counts/offsets are in
 * 32-bit words. */
typedef struct nx_comm {
    int32_t rank, world;
    void* user;
    int (*send)(void* user, int32_t dst, const uint32_t* d_buf, size_t n_words);          /* device buffer (ring commit protocol only) */
    int (*recv)(void* user, int32_t src, uint32_t* d_buf, size_t n_words);                /* device buffer (ring commit protocol only) */
    int (*allreduce_m31)(void* user, uint32_t* d_buf, size_t n_words);                    /* unused by the row-sharded prove          */
    int (*allgather)(void* user, const void* h_send, size_t bytes, void* h_recv);         /* host: recv = world x bytes               */
    int (*broadcast)(void* user, void* h_buf, size_t bytes, int32_t root);                /* host (unused by the row-sharded prove)   */
    /* device all-to-all: words [send_off[r], send_off[r] + send_cnt[r]) of d_send go to rank r; what rank r sent lands at
     * [recv_off[r], recv_off[r] + recv_cnt[r]) of d_recv (arrays of `world` entries; the own share is copied too).  d_send is complete
     * on entry, d_recv must be complete on return; OTHER work of the library may still be queued on the context's stream (the next
     * column chunk's transforms), so run the collective on a stream of the transport's own and wait for that stream only */
    int (*alltoallv)(void* user, const uint32_t* d_send, const size_t* send_off, const size_t* send_cnt, uint32_t* d_recv,
                     const size_t* recv_off, const size_t* recv_cnt);
    /* device all-gather: d_recv = world x n_words, rank r's contribution at r * n_words */
    int (*allgather_dev)(void* user, const uint32_t* d_send, size_t n_words, uint32_t* d_recv);
    /* optional (may be NULL).  The library calls it on a rank whose prove FAILED after the exchanges of a proof may have started (a
     * HIP error, out of memory, a failed callback): its peers are, or will be, waiting for it in a collective it will never enter.
     * The transport must make the pending and later collectives of this communicator fail on the peers instead of waiting — tear the
     * group down (the thread-rank transport breaks its barrier; the native RCCL transport calls ncclCommAbort and, since RCCL does
     * not propagate that to live peers, additionally bounds every wait by the context option "comm.timeout_ms").  A communicator
     * is unusable after abort. */
    void (*abort)(void* user);
} nx_comm;
/* The native transport: RCCL over xGMI (csrc/comm_rccl.hip; librccl is opened at run time, NX_ERR_HIP when it is not there).  Rank 0
 * calls nx_rccl_unique_id and ships the 128 bytes to the other ranks through any side channel (environment, file, socket — the
 * bootstrap every NCCL program has); every rank then creates its communicator on its own context and hands `*out` to the prove
 * entries / nx_prover_set_comm.  Collectives run on a stream of the transport's own (see alltoallv above).  One process or thread
 * per GPU; RCCL itself refuses two ranks on one device. */
int nx_rccl_unique_id(uint8_t id[128]);
int nx_comm_rccl_create(nx_ctx* ctx, const uint8_t unique_id[128], int32_t rank, int32_t world, nx_comm** out);
void nx_comm_rccl_destroy(nx_comm* comm);
/* The in-process transport (csrc/comm_local.hip): ONE process drives the GPUs of a node with one thread per GPU — each thread its own
 * context and its own communicator of one shared group — and the collectives are rendezvous of those threads plus device-to-device copies
 * every rank pulls from its peers (peer to peer over xGMI between two devices; plain copies when several contexts share one GPU, which is
 * how the test-suite runs the 2 / 4 / 8-rank proofs on a one-GPU box).  No RCCL, no second process.  abort() breaks the group: every
 * waiting and later collective fails on every rank; waits are bounded by "comm.timeout_ms".  The group outlives its communicators. */
typedef struct nx_comm_group nx_comm_group;
int nx_comm_group_create(int32_t world, nx_comm_group** out);
void nx_comm_group_destroy(nx_comm_group* group);
/* A group that a failure broke (abort, a timeout) stays broken until it is re-armed: call this when EVERY rank's thread has returned
 * from its prove call (refused while a rank is still copying).  The prove entries abort only on failures that can leave peers waiting
 * — a HIP / transport / allocation error on one rank —; a refusal every rank reaches by itself (an argument error, the vote before the
 * first exchange, ProvingError::ConstraintsNotSatisfied from the all-gathered sampled values) leaves the group and an RCCL
 * communicator usable for the next proof. */
int nx_comm_group_reset(nx_comm_group* group);
int nx_comm_group_broken(const nx_comm_group* group);
/* 1: rank `from_rank` pulls from `to_rank`'s device peer to peer (xGMI) or they share a device; 0: the runtime stages those copies
 * (peer access could not be enabled); -1: one of the two communicators does not exist yet. */
int nx_comm_group_peer_access(nx_comm_group* group, int32_t from_rank, int32_t to_rank);
int nx_comm_local_create(nx_comm_group* group, nx_ctx* ctx, int32_t rank, nx_comm** out);
void nx_comm_local_destroy(nx_comm* comm);
/* Which columns of a tree a GPU transforms: groups = (column count, log size) per component in commit order; consecutive groups
 * of one size form a run whose columns are cut into `world` contiguous balanced ranges; lo/hi[i] = this rank's [lo, hi) of group i.
 * Host arithmetic only (no context, no GPU). */
int nx_plan_local_columns(const uint32_t* group_n_cols, const uint32_t* group_log_sizes, uint32_t n_groups, int32_t rank,
                          int32_t world, uint32_t* lo, uint32_t* hi);
/* nx_prove_synth on the GPUs of `comm`. */
int nx_prove_synth_sharded(nx_ctx* ctx, const nx_component_spec* comps, uint32_t n_comps, const nx_pcs_config* cfg,
                           uint64_t seed, const uint8_t* ad, size_t ad_len, const nx_comm* comm, uint32_t** proof_words,
                           size_t* n_words, nx_prove_stats* stats);
/* Modular add / widening helpers for transports that sum M31 buffers (RCCL has no modular reduction). */
int nx_m31_add_into(nx_ctx* ctx, uint32_t* d_dst, const uint32_t* d_src, size_t n_words);
int nx_m31_widen(nx_ctx* ctx, uint64_t* d_dst, const uint32_t* d_src, size_t n_words);
int nx_m31_narrow(nx_ctx* ctx, uint32_t* d_dst, const uint64_t* d_src, size_t n_words);

/* ------------------------------------------- "next" row R9: recorded AIR constraints evaluated on device ---------------
 * The reference's AIR closures (MachineEval::evaluate, prover/src/components/mod.rs:39-57; BuiltInComponentEval::evaluate,
 * prover2/machine/src/framework/eval.rs:19-33) cannot cross a C ABI, but a recording EvalAtRow — the trick Stwo's
 * InfoEvaluator already plays to discover masks (prover/src/components/mod.rs:59-67) — turns them into a straight-line
 * program over the field tower, and that can.  Registers are indices of a per-row register file (a secure-field value takes
 * 4 consecutive registers); the host allocates them.  For every row of the evaluation domain (bit-reversed circle-domain
 * order, log size log_eval) the program runs once and  acc[row] += (sum_j alpha_powers[j] * C_j(row)) * denom_inv[row >> log_size]
 * (FrameworkComponent::evaluate_constraint_quotients_on_domain).
 * Row offsets (NX_C_LOAD, NX_C_LOADE): any int32 is allowed and is taken modulo the trace length 2^log_size — row + b trace steps is
 * natural trace row (i + b) mod 2^log_size, on every evaluation domain.  Tested on the device against the oracle at offsets beyond
 * +-1, of the trace length and more, and at INT32_MIN / INT32_MAX (tests/test_gpu_wide_masks.py). */
enum {
    NX_C_LOAD = 0,          /* B[dst] = cols[a][row + (int32)b trace steps]                          */
    NX_C_CONST = 1,         /* B[dst] = a (canonical M31 immediate)                                  */
    NX_C_ADD = 2, NX_C_SUB = 3, NX_C_MUL = 4, /* B[dst] = B[a] op B[b]                               */
    NX_C_NEG = 5,           /* B[dst] = -B[a]                                                        */
    NX_C_CONSTE = 6,        /* E[dst] = econsts[a]   (QM31: lookup elements, ...)                    */
    NX_C_ADDE = 7, NX_C_SUBE = 8, NX_C_MULE = 9, /* E[dst] = E[a] op E[b]                            */
    NX_C_MULEB = 10,        /* E[dst] = E[a] * B[b]                                                  */
    NX_C_ADDEB = 11,        /* E[dst] = E[a] + B[b]                                                  */
    NX_C_LOADE = 12,        /* E[dst] = (cols[a], cols[a+1], cols[a+2], cols[a+3])[row + (int32)b steps]  (a secure column) */
    NX_C_CONSTRAINT_B = 13, /* add_constraint(B[a])                                                  */
    NX_C_CONSTRAINT_E = 14, /* add_constraint(E[a])                                                  */
    /* logup FRACTION programs only (nx_logup_program): a relation entry of the AIR, add_to_relation(RelationEntry { relation,
     * multiplicity, values }) — numerator = the multiplicity expression, denominator = relation.combine(values) */
    NX_C_FRAC = 15,         /* fraction E[a] / E[b] of logup column (batch) dst                       */
    NX_C_FRACB = 16         /* fraction B[a] / E[b] of logup column (batch) dst (a base-field numerator) */
};
typedef struct nx_cinstr { uint32_t op, dst, a, b; } nx_cinstr;
int nx_eval_constraint_program(nx_ctx* ctx, const nx_cinstr* program, uint32_t n_instr, uint32_t n_regs,
                               const uint32_t* const* d_cols, uint32_t n_cols, const uint32_t* econsts /* 4 words each */,
                               uint32_t n_econsts, const uint32_t* alpha_powers /* 4 words per constraint */,
                               uint32_t n_constraints, const uint32_t* denom_inv /* 2^(log_eval-log_size) words */,
                               uint32_t log_size, uint32_t log_eval, uint32_t* const* d_acc4);

/* The same program compiled into a gfx950 kernel at run time (hiprtc): straight-line code over VGPRs instead of an LDS
 * register file, ~3x faster than the interpreter; lookup elements and alpha powers stay run-time arguments, so one compilation
 * serves every proof of an AIR.  h_source_out (optional, may be the only output: then ctx may be NULL and no GPU is needed)
 * receives the generated HIP source (free with nx_free_host).  nx_air_eval is stream-ordered like the other kernels: it returns
 * once the launch is enqueued (nx_sync or any later entry that reads the accumulator orders after it). */
typedef struct nx_air_kernel nx_air_kernel;
int nx_air_compile(nx_ctx* ctx, const nx_cinstr* program, uint32_t n_instr, uint32_t n_regs, uint32_t n_cols,
                   uint32_t n_econsts, uint32_t n_constraints, nx_air_kernel** out, char** h_source_out);
int nx_air_eval(nx_ctx* ctx, const nx_air_kernel* kernel, const uint32_t* const* d_cols, const uint32_t* econsts,
                const uint32_t* alpha_powers, const uint32_t* denom_inv, uint32_t log_size, uint32_t log_eval,
                uint32_t* const* d_acc4);
void nx_air_kernel_destroy(nx_air_kernel* kernel);
/* Ahead-of-time kernels: the hiprtc compilation of a recorded AIR costs from 0.7 s (the bench's AIR) to seconds (a keccak-shaped one) and
 * would otherwise be paid by the first proof of every process.
 * nx_air_kernel_save: the kernel as a self-describing blob (header + gfx950 code object; free with nx_free_host) — build it once, in a
 * build step or on another box, ship it; nx_air_kernel_load: a kernel from such a blob, in milliseconds (checksummed; a blob of another
 * library version is refused).  Pass the loaded kernel in nx_air_component.kernel.
 * nx_air_cache_dir: a directory (created if its parent exists; NULL or "" = off; initial value: the environment variable
 * NX_AIR_CACHE_DIR) in which the library keeps those blobs by itself, keyed by a hash of the generated source, the target and the hiprtc
 * version: nx_air_compile / nx_air_compile_subset — and therefore the provers, which compile their components' kernels through them —
 * load from it when they can and store what they compile (write-then-rename, one temporary per writer: processes and threads may
 * share a directory).  Process-wide.  The directory is TRUSTED INPUT — its files are GPU code objects, accepted on a 64-bit checksum, not a
 * signature: it is created with mode 0700 and ignored (with one line on stderr) unless it is a directory owned by the calling user that
 * neither group nor others may write to.
 * nx_air_cache_stats: kernels compiled by hiprtc / loaded from the directory / stored into it by this process (any pointer may be NULL).
 * COMPILATION IN PROCESSES: a generated source of >= 4 kernels is cut into one part per kernel and the parts are compiled side by side by
 * helper processes — the executable nx_air_cc next to this library (environment NX_AIR_CC: another path), at most NX_AIR_COMPILE_PROCS at a
 * time (default: the host's hardware threads, at most 32; 1 = everything in this process).  hiprtc serialises the threads of a process, not
 * processes: the first proof of the keccak-shaped statement waits 2.1 s instead of 14 s (profiles/r06_compile_procs.jsonl).  The blob is
 * the same bytes however it was compiled; without the helper the parts go through hiprtc here. */
int nx_air_kernel_save(const nx_air_kernel* kernel, uint8_t** blob, size_t* n_bytes);
int nx_air_kernel_load(nx_ctx* ctx, const uint8_t* blob, size_t n_bytes, nx_air_kernel** out);
int nx_air_cache_dir(const char* dir);
int nx_air_cache_stats(uint64_t* n_compiled, uint64_t* n_disk_hits, uint64_t* n_stored);
/* Degree-aware evaluation.  FrameworkEval::max_constraint_log_degree_bound (reference prover/src/components/mod.rs:44-45: +2 for v1's
 * main component) is the bound of the component's HIGHEST-degree constraint: Stwo evaluates every constraint, and therefore
 * re-extends every column, on the domain of log_size + bound.  A constraint of degree d over columns of 2^n rows has its quotient in
 * the FFT space of 2^(n+e) points iff d <= 2^e + 1, so the constraints of degree <= 3 (v1: all the logup constraints of
 * finalize_logup, components/mod.rs:53, i.e. all 1000 interaction columns; most chip constraints) can be evaluated on the
 * 2^(n+1)-point domain — with blowup 2 the committed evaluations, no re-extension — and lifted like a smaller component
 * (DomainEvaluationAccumulator::finalize); the composition polynomial, and the proof, are the same bits.
 * nx_air_constraint_degrees: an upper bound of every constraint's degree (host only; ctx may be NULL).
 * nx_air_compile_subset: nx_air_compile for the constraints with select[j] != 0 (NULL = all) — same alpha-power and column
 * indices as the whole program, so kernels of disjoint subsets add up to the whole; columns no selected constraint loads may be
 * NULL in nx_air_eval's d_cols.  The prover does this by itself (context option "air.degree_split", default 1). */
int nx_air_constraint_degrees(nx_ctx* ctx, const nx_cinstr* program, uint32_t n_instr, uint32_t n_regs, uint32_t n_cols,
                              uint32_t n_econsts, uint32_t n_constraints, uint32_t* degrees /* n_constraints */);
int nx_air_compile_subset(nx_ctx* ctx, const nx_cinstr* program, uint32_t n_instr, uint32_t n_regs, uint32_t n_cols,
                          uint32_t n_econsts, uint32_t n_constraints, const uint8_t* select /* n_constraints, or NULL */,
                          nx_air_kernel** out, char** h_source_out);

/* ------------------------------------------- the prover session: stwo::prover::prove over recorded AIRs
 * What `nexus_vm_prover::prove` does around Stwo (reference prover/src/machine.rs:184-296; prover2/machine/src/prove.rs) with
 * the AIR supplied as recorded constraint programs instead of Rust closures.  The caller replays the reference's transcript
 * prefix through the session — mix the program description (machine.rs:198-206), commit the preprocessed tree (:208-228) and the
 * main tree (:230-237), draw lookup elements (:239-240), build the interaction trace (nx_logup_*), mix the claimed sums (:262),
 * commit the interaction tree (:263) — and nx_prover_prove runs CommitmentSchemeProver / stwo::prover::prove (:286-290) on the
 * device: composition polynomial (nx_air_eval), OODS sampling, DEEP quotients, FRI, proof of work, decommitment.  The proof is
 * in the NXP1 word format of nx_prove_synth.  The session proves the trace trees it was given — the reference commits three
 * (preprocessed, main, interaction), Stwo's prove takes any TreeVec; a component column names its tree by index —; the composition
 * polynomial's tree follows them. */
typedef struct nx_prover nx_prover;
int nx_prover_create(nx_ctx* ctx, const nx_pcs_config* cfg, uint32_t max_log_size, nx_prover** out);
void nx_prover_destroy(nx_prover* prover);
/* One proof on several GPUs: every GPU runs the same session calls with its own communicator (see nx_comm); nx_prover_tree_begin
 * then hands each GPU only ITS columns (NULL for the others).  Call right after nx_prover_create. */
int nx_prover_set_comm(nx_prover* prover, const nx_comm* comm);
/* Blake2sChannel of the session */
int nx_prover_mix_u64(nx_prover* prover, uint64_t v);
int nx_prover_mix_felts(nx_prover* prover, const uint32_t* felts, uint32_t n_felts); /* 4 words per QM31 */
int nx_prover_draw_felt(nx_prover* prover, uint32_t out[4]);
/* Channel::draw_felts(n): n secure felts from the base-felt stream (two per Blake2s draw) — LookupElements::draw's (z, alpha) */
int nx_prover_draw_felts(nx_prover* prover, uint32_t n_felts, uint32_t* out /* 4 words each */);
int nx_prover_channel_digest(const nx_prover* prover, uint8_t digest[32]);
/* TreeBuilder::extend_evals + commit (machine.rs:208-263).  tree_begin allocates the tree's columns in the session (one slab per
 * run of equal log sizes) and returns their device addresses; the caller fills them with bit-reversed circle-domain evaluations
 * (trace generation on the device, nx_upload_columns, nx_copy ...); tree_commit interpolates, extends, commits and mixes the root.
 * The columns then belong to the session (they hold the coefficients afterwards). */
int nx_prover_tree_begin(nx_prover* prover, const uint32_t* log_sizes, uint32_t n_cols, uint32_t** d_cols_out);
int nx_prover_tree_commit(nx_prover* prover, uint8_t root[32]);
/* The same for a tree whose columns are in HOST memory — what the reference's trace builder hands over (`Vec<Vec<M31>>`,
 * prover/src/trace/trace_builder.rs:19-32): h_cols[i] is the host source of column i of the tree begun with nx_prover_tree_begin
 * (2^log_sizes[i] words; natural coset order when coset_order != 0 — R3's permutation then runs on the device — else bit-reversed
 * circle-domain order).  The commit uploads the columns in chunks on a copy stream and transforms each chunk as soon as it has arrived:
 * PCIe transfer, iFFT + LDE and leaf hashing overlap.  keep_idx / d_keep (n_keep entries, may be 0):
 * columns whose EVALUATIONS are needed after the commit (the logup fractions read main-trace columns; the commit turns columns into
 * coefficients in place) are cloned into d_keep[k] (2^log words, caller-allocated) on arrival — the reference's whole-trace clone
 * (machine.rs:232), for the columns that need it.  Blocking like nx_prover_tree_commit; the host columns are free on return.
 * A row-sharded session uploads its own columns first (no overlap) and commits as usual. */
int nx_prover_tree_commit_host(nx_prover* prover, const uint32_t* const* h_cols, int coset_order, const uint32_t* keep_idx,
                               uint32_t n_keep, uint32_t* const* d_keep, uint8_t root[32]);
/* nx_prover_tree_commit_host with an element kind per host column (kinds[i] for h_cols[i], NX_COL_*; NULL = all NX_COL_U32): the
 * reference's byte-limb trace columns (TracesBuilder, trace_builder.rs:19-32) cross PCIe as bytes and are widened on the device under
 * the commit's transforms; nx_upload_columns_narrow describes the kinds, the pinning and the refusal.  A refused value returns NX_ERR_ARG
 * before the root is mixed: the transcript is untouched, the tree is no longer begun, and the caller may nx_prover_tree_begin the same
 * tree again and commit corrected columns — the proof is then the one that never saw the refusal.  Blocking; the host columns are free
 * on return.  A row-sharded session uploads its own columns through nx_upload_columns_narrow first, as the u32 form does. */
int nx_prover_tree_commit_host_narrow(nx_prover* prover, const void* const* h_cols, const uint8_t* kinds, int coset_order,
                                      const uint32_t* keep_idx, uint32_t n_keep, uint32_t* const* d_keep, uint8_t root[32]);
/* A committed tree that is proved over and over — the preprocessed tree: the reference commits the same preprocessed + program columns
 * in every proof of a program (prover/src/machine.rs:208-228) and once more in every verification (machine.rs:363-417, verify.rs:103-143,
 * which needs only the root) — need not be transformed and hashed again.  nx_prover_tree_share turns committed tree `tree_index` of a
 * session into a reference-counted handle (the session keeps proving with it); nx_prover_tree_adopt makes it the NEXT tree of another
 * session of the SAME context and mixes its root, exactly as nx_prover_tree_commit would after a fresh commit of the same columns: the
 * proof bytes are those of the fresh commit.  After a commit a tree's buffers are read-only, so any number of sessions may hold one.
 * One GPU; same blowup factor and node hash.  nx_committed_tree_release drops the handle (the buffers go when the last session that
 * adopted it is destroyed); nx_committed_tree_root: the root and the column count (a verifier's preprocessed-root check).
 * LIFETIME: a handle and every session that adopted it belong to the context that committed the tree — release / destroy them BEFORE
 * nx_ctx_destroy (their buffers return to that context's allocator; afterwards the handle dangles). */
typedef struct nx_committed_tree nx_committed_tree;
int nx_prover_tree_share(nx_prover* prover, uint32_t tree_index, nx_committed_tree** out);
int nx_prover_tree_adopt(nx_prover* prover, const nx_committed_tree* tree, uint8_t root[32]);
int nx_committed_tree_root(const nx_committed_tree* tree, uint8_t root[32], uint32_t* n_cols);
void nx_committed_tree_release(nx_committed_tree* tree);
/* A component: what FrameworkComponent<E> is to Stwo (reference prover/src/components/mod.rs:15-57).  Column k of the program is
 * column col_index[k] of tree col_tree[k] (TraceLocationAllocator); it is sampled at the mask_count[k] row offsets listed next in
 * mask_offsets (InfoEvaluator, components/mod.rs:59-67) — every LOAD offset must be listed, every committed column must be
 * claimed by some component.  kernel: the program compiled by nx_air_compile, or NULL to let nx_prover_prove compile it.
 * A mask offset is any int32, taken modulo the trace length: the column is sampled at the OODS point + offset trace steps.  Two entries
 * of one column that coincide modulo the length are sampled twice at the same point (two equal values in the proof, one quotient batch
 * holding the column twice); tested with the rest of the wide offsets (tests/test_gpu_wide_masks.py). */
typedef struct {
    uint32_t log_size;
    const nx_cinstr* program; uint32_t n_instr, n_regs;
    const uint32_t* econsts; uint32_t n_econsts;
    uint32_t n_constraints;
    const uint32_t* col_tree; const uint32_t* col_index; uint32_t n_cols;
    const uint32_t* mask_count; const int32_t* mask_offsets;
    const nx_air_kernel* kernel;
    uint32_t log_constraint_degree_bound;   /* this component's bound (see nx_component_spec): 0 = the session config's log_constraint_degree */
} nx_air_component;
/* stwo::prover::prove.  NX_ERR_PROTOCOL = ProvingError::ConstraintsNotSatisfied.  *proof_words: free with nx_free_host.  After a proof
 * nx_prover_channel_digest is the transcript's final state; another nx_prover_prove starts again from the state the first one found
 * (and a failed call restores it at once), so proving the committed statement again — or retrying — gives the same bytes. */
int nx_prover_prove(nx_prover* prover, const nx_air_component* components, uint32_t n_components, uint32_t** proof_words,
                    size_t* n_words, nx_prove_stats* stats);

/* ------------------------------------------- the trace checker: stwo_constraint_framework::assert_constraints_on_polys on the device
 * The reference's day-to-day tool for the author of an AIR or of a trace (prover/src/test_utils.rs:113-168 assert_chip, the tests of
 * every prover2 component): every constraint on every row of the TRACE domain, and the first one that is not zero named.  nx_prover_prove
 * can only say ConstraintsNotSatisfied — by then all constraints of all components are folded into one random linear combination.
 * SEMANTICS.  Domain: CanonicCoset(log_size).circle_domain() of the component, i.e. the 2^log_size rows the caller filled (not the
 * committed extension, which does not contain them).  Rows in every report are NATURAL trace rows i (coset order, the VM step), not
 * storage positions: position pos of the bit-reversed circle-domain order holds row d < N/2 ? 2d : 2N-1-2d with d = bitrev(pos).  A LOAD /
 * LOADE with offset o at row i reads row (i + o) mod N.  A base-field constraint fails at a row where it is not 0, a secure one where
 * any of its four coordinates is not 0.  The logup claimed-sum consistency is part of the recorded program (the [-1, 0] constraint).
 * Per failing constraint: how many rows fail, the smallest such row, the constraint's value there.  The counts are integers combined
 * with add and min: the report is the same on every run, whatever the scheduling. */
typedef struct nx_check_failure {
    uint32_t component, constraint;   /* index into the component array; ordinal of the add_constraint */
    uint32_t first_row;               /* smallest natural trace row at which it is not zero            */
    uint32_t value[4];                /* its value there (a base-field constraint: value[1..3] = 0)    */
    uint64_t n_rows;                  /* rows at which it is not zero                                  */
} nx_check_failure;
/* The primitive: one recorded program over d_cols, TRACE-DOMAIN EVALUATIONS (bit-reversed circle-domain order, 2^log_size words each —
 * what nx_prover_tree_begin hands out, before the commit; columns no constraint loads may be NULL).  Writes min(cap, failing) entries
 * in ascending constraint order (component = 0) and the number of failing constraints to *n_failed.  The program's check kernels are
 * compiled by hiprtc on first use and kept per context, keyed by the program bytes (nx_air_cache_dir applies).  A valid trace costs
 * one pass over the loaded columns: no atomic, nothing stored to memory (failing rows are reduced per wave, then per block in LDS,
 * then one atomic pair per block and failing constraint).  Blocking.
 * Returns NX_OK when every constraint holds on every row; NX_ERR_PROTOCOL when at least one fails — nx_last_error then names the first
 * one, "component 0 constraint 2: not zero on 1 of 64 rows, first at row 47" — with the array and the count filled in both cases; any
 * other code is an ordinary error and leaves them untouched.
 * nx_air_check_source: the HIP source of those kernels (host only, no context, no GPU; free with nx_free_host). */
int nx_air_check(nx_ctx* ctx, const struct nx_cinstr* program, uint32_t n_instr, uint32_t n_regs, const uint32_t* const* d_cols,
                 uint32_t n_cols, const uint32_t* econsts, uint32_t n_econsts, uint32_t n_constraints, uint32_t log_size,
                 nx_check_failure* failures, uint32_t cap, uint32_t* n_failed);
int nx_air_check_source(const struct nx_cinstr* program, uint32_t n_instr, uint32_t n_regs, uint32_t n_cols, uint32_t n_econsts,
                        uint32_t n_constraints, char** h_source_out);
/* The session form: the component array of nx_prover_prove, once the trees the components name are committed; any number of times,
 * before or after nx_prover_prove.  Reads the session only: the transcript (nx_prover_channel_digest) and the proof a later
 * nx_prover_prove returns are unchanged.  The committed columns hold coefficients, so the columns a component's constraints load are
 * evaluated on its trace domain into scratch, checked, and freed before the next component.  Entries in (component, constraint) order.
 * DEVICE MEMORY: peak above the session's  <=  4 * 2^log_size * (columns the constraints load)  of the largest component, plus
 * 24 bytes per column and constraint for the tables and, on the failing path only, 20 bytes per loaded word of every distinct
 * reported first row (value[] is computed on the host from those words); each term rounded up to 256.  Nothing is kept afterwards.
 * Statement errors (a column claimed by no component, a LOAD offset missing from the mask, a column outside the committed trees ...)
 * are NX_ERR_ARG with nx_prover_prove's texts.  A session with a communicator is refused (NX_ERR_ARG, "one GPU").  Returns as nx_air_check. */
int nx_prover_check(nx_prover* prover, const nx_air_component* components, uint32_t n_components, nx_check_failure* failures,
                    uint32_t cap, uint32_t* n_failed);

/* ------------------------------------------- the verifier session: core::verifier::verify over recorded AIRs
 * `nexus_vm_prover::verify` (reference prover/src/lib.rs:26-33; prover/src/machine.rs:299-485; prover2/machine/src/verify.rs:28-143)
 * around Stwo's core::verifier::verify, CommitmentSchemeVerifier, FriVerifier and MerkleVerifier, mirroring the prover session one to
 * one: the caller replays the transcript prefix — mix the program description (machine.rs:437-446), commit the preprocessed root
 * (:447-449, verify.rs:60-70), the main root, draw the lookup elements (:451), mix the claimed sums (:448-450 of the prover's order,
 * machine.rs:262), commit the interaction root — and nx_verifier_verify checks the proof.
 * HOST ONLY: the verifier is KBs of hashing and a few hundred field operations whatever the trace size; it takes no context and runs in
 * a process that sees no GPU (nx_ctx_create fails there with NX_ERR_NO_DEVICE).  The node-hash rule a context otherwise holds is the
 * hash_mode argument (NX_HASH_*; cfg->hash_mode is NOT read).  The one step whose cost grows with the trace — re-committing the
 * preprocessed columns to compare the root (machine.rs:363-417, verify.rs:103-143) — is nx_commit_root below, on the device.
 * Returns: NX_OK accepted; NX_ERR_VERIFY a well-formed proof failed a check; NX_ERR_ARG words that cannot be parsed (truncated, a count
 * beyond the stream, a field word >= p, trailing words) or an inconsistent statement.  nx_verifier_last_error names the failing check
 * ("tree 1: Merkle root mismatch", "proof of work", "FRI layer 3: Merkle root mismatch" ...).
 * UNTRUSTED INPUT: proof words come from outside; every count in the stream is bounded by the remaining words and by the statement
 * before anything is allocated or indexed. */
typedef struct nx_verifier nx_verifier;
int nx_verifier_create(const nx_pcs_config* cfg, int hash_mode, nx_verifier** out);
void nx_verifier_destroy(nx_verifier* verifier);
const char* nx_verifier_last_error(const nx_verifier* verifier);
/* Blake2sChannel of the session: as nx_prover_mix_u64 / _mix_felts / _draw_felt / _draw_felts / _channel_digest */
int nx_verifier_mix_u64(nx_verifier* verifier, uint64_t v);
int nx_verifier_mix_felts(nx_verifier* verifier, const uint32_t* felts, uint32_t n_felts);
int nx_verifier_draw_felt(nx_verifier* verifier, uint32_t out[4]);
int nx_verifier_draw_felts(nx_verifier* verifier, uint32_t n_felts, uint32_t* out);
int nx_verifier_channel_digest(const nx_verifier* verifier, uint8_t digest[32]);
/* CommitmentSchemeVerifier::commit (machine.rs:447-482): the root of the next tree and its columns' log sizes (the trace sizes, as
 * nx_prover_tree_begin takes them); mixes the root. */
int nx_verifier_tree_commit(nx_verifier* verifier, const uint8_t root[32], const uint32_t* log_sizes, uint32_t n_cols);
/* The same with the root COMPUTED from the columns on the device (nx_commit_root): the verifier's re-commit of the preprocessed trace
 * (machine.rs:363-417; verify.rs:103-143).  d_cols as nx_commit_root takes them (consumed: they hold coefficients afterwards).  The
 * context's hash mode must be the session's. */
int nx_verifier_tree_commit_columns(nx_verifier* verifier, nx_ctx* ctx, const nx_twiddles* tw, uint32_t* const* d_cols, const uint32_t* log_sizes,
                                    uint32_t n_cols, uint8_t root[32]);
/* core::verifier::verify (machine.rs:483-485, verify.rs:134-143) of an NXP1 proof against the committed roots: the same component array
 * nx_prover_prove takes (`kernel` is ignored); every recorded program runs once, at the out-of-domain point, over QM31 on the host.
 * Checks, in order: the proof's shape against the committed column sizes and masks; the commitments against the committed roots; the
 * composition value at the out-of-domain point; the FRI commit phase replayed on the channel (both fri_alpha_mode values); proof of
 * work; query positions; every Merkle decommitment (both node-hash rules, mixed-degree trees); the DEEP quotients at the queried
 * positions; every FRI layer and the last-layer polynomial.  After NX_OK nx_verifier_channel_digest is the transcript's final state;
 * another call starts again from the state the first one found and a refusal restores it at once, so verifying again gives the same
 * answer. */
int nx_verifier_verify(nx_verifier* verifier, const nx_air_component* components, uint32_t n_components, const uint32_t* proof_words,
                       size_t n_words);
/* `nexus_vm_prover::verify` for the machine of nx_prove_machine (machine.rs:363-500): replays the transcript prefix as nx_prove_machine
 * writes it (ad bytes, log sizes, the preprocessed and main roots out of the proof, lookup elements drawn, claimed sums mixed, the
 * interaction root), rebuilds the components from the drawn elements and the claimed sums (4 words per component: `Proof.claimed_sum`,
 * nx_machine_claimed_sums) with nx_machine_air_program's emitter, and verifies.  expected_logup_sum (4 words, or NULL): the value the
 * claimed sums must add up to — verify_logup_sum (prover2/machine/src/verify.rs:145-160) compares their sum with the memory boundary's
 * expected sum, a function of public data; the synthetic machine has no such public value, so its caller passes the sum it expects or
 * NULL for no check.  A caller that also holds the preprocessed columns compares proof root 0 with nx_commit_root of them.
 * err_text (optional, err_cap bytes): the failing check.  Host only. */
int nx_verify_machine(const nx_component_spec* comps, uint32_t n_comps, const nx_pcs_config* cfg, int hash_mode, const uint8_t* ad,
                      size_t ad_len, const uint32_t* proof_words, size_t n_words, const uint32_t* claimed_sums,
                      const uint32_t* expected_logup_sum, char* err_text, size_t err_cap);
/* The counterpart of nx_prove_synth: its transcript prefix and the synthetic AIR's constraints evaluated at the out-of-domain point on
 * the host (the proving side has them as a device kernel only).  Host only. */
int nx_verify_synth(const nx_component_spec* comps, uint32_t n_comps, const nx_pcs_config* cfg, int hash_mode, const uint8_t* ad,
                    size_t ad_len, const uint32_t* proof_words, size_t n_words, char* err_text, size_t err_cap);

/* ------------------------------------------- "next" row R8: logup interaction trace on device ------------------------
 * The reference fills the interaction trace on the CPU (prover/src/traits.rs:124-145 generate_interaction_trace -> per chip,
 * e.g. prover/src/chips/range_check/range256.rs:271-288; prover2/machine/src/lookups/logup_trace_builder.rs:22-121) through
 * stwo-constraint-framework's LogupTraceGenerator.  For main-trace columns that already live in HBM: */
/* Relation::combine: denom(row) = sum_i alpha_powers[i] * tuple_i(row) - z   (alpha_powers: 4 words per tuple column) */
int nx_logup_combine(nx_ctx* ctx, const uint32_t* const* d_tuple_cols, uint32_t n_cols, const uint32_t* alpha_powers,
                     const uint32_t z[4], uint32_t log_size, uint32_t* const* d_out4);
/* LogupColGenerator::{write_frac, finalize_col}: out(row) = num/den + prev(row).  A numerator is scale * mult(row)
 * (d_mult NULL: the constant `scale`, e.g. 1 or -1).  With a second fraction (d_den_b4 != NULL) the two are merged first,
 * (a d + b c) / (b d), as prover2's LogupTraceBuilder::add_to_relation_with does (logup_trace_builder.rs:93-97).
 * d_prev4 NULL for the first column.  out may alias prev. */
int nx_logup_finalize_col(nx_ctx* ctx, uint32_t log_size, const uint32_t* d_mult_a, const uint32_t scale_a[4],
                          const uint32_t* const* d_den_a4, const uint32_t* d_mult_b, const uint32_t scale_b[4],
                          const uint32_t* const* d_den_b4, const uint32_t* const* d_prev4, uint32_t* const* d_out4);
/* Fused form of the two calls above (the denominators never touch memory): one interaction column from one or two
 * fractions given by their tuple columns.  frac_b NULL = a single fraction; d_prev4 NULL = the first column. */
typedef struct nx_logup_frac {
    const uint32_t* const* d_tuple_cols; uint32_t n_tuple_cols;   /* relation tuple (main-trace columns)                */
    const uint32_t* alpha_powers;                                 /* 4 words per tuple column                           */
    const uint32_t* z;                                            /* 4 words                                            */
    const uint32_t* d_mult;                                       /* multiplicity column or NULL                        */
    const uint32_t* scale;                                        /* 4 words: numerator = scale * mult (or scale)       */
} nx_logup_frac;
int nx_logup_col(nx_ctx* ctx, uint32_t log_size, const nx_logup_frac* frac_a, const nx_logup_frac* frac_b,
                 const uint32_t* const* d_prev4, uint32_t* const* d_out4);
/* The n_cols logup columns of a component in ONE launch: column j = sum over i <= j of fraction i(row), i.e. what n_cols calls of
 * nx_logup_col with d_prev4 = the previous column produce, reading every tuple column once.  d_out: 4 n_cols coordinate columns. */
int nx_logup_cols(nx_ctx* ctx, uint32_t log_size, const nx_logup_frac* fracs, uint32_t n_cols, uint32_t* const* d_out);
/* The general form, stwo-constraint-framework's finalize_logup_batched on the trace side: fraction i belongs to batch batching[i]
 * (any order; every batch 0 .. n_cols - 1 must hold at least one fraction), column j = sum of the fractions of batches <= j — the
 * merged fraction (a d + b c) / (b d) of a pair (LogupTraceBuilder::add_to_relation_with, reference prover2/machine/src/lookups/
 * logup_trace_builder.rs:86-101) is the sum of its two fractions.  batching NULL = in pairs (i / 2: finalize_logup_in_pairs; an odd
 * n_fracs leaves the last column one fraction).  One launch; every tuple column is read once.  d_out: 4 n_cols coordinate columns. */
int nx_logup_cols_batched(nx_ctx* ctx, uint32_t log_size, const nx_logup_frac* fracs, uint32_t n_fracs, const uint32_t* batching,
                          uint32_t n_cols, uint32_t* const* d_out);
/* LogupTraceGenerator::finalize_last on the last column (in place): claimed_sum = sum over all rows; the column becomes
 * the inclusive prefix sum, in natural coset order, of (value - claimed_sum / 2^log_size). */
int nx_logup_finalize_last(nx_ctx* ctx, uint32_t log_size, uint32_t* const* d_col4, uint32_t claimed_sum[4]);
/* The same for n_cols secure columns of one size (d_cols4: n_cols x 4 coordinate pointers; claimed_sums: n_cols x 4 words) in three
 * launches and one device-to-host copy: the form for AIRs with many components / logup columns (BASELINE config #5). */
int nx_logup_finalize_last_batch(nx_ctx* ctx, uint32_t log_size, uint32_t* const* d_cols4, uint32_t n_cols,
                                 uint32_t* claimed_sums);

/* The interaction trace of a component FROM ITS RECORDED AIR.  A recording EvalAtRow sees every relation entry the AIR declares —
 * eval.add_to_relation(RelationEntry::new(relation, multiplicity, &values)), e.g. reference prover/src/components/mod.rs:48-56,
 * prover/src/extensions/keccak/round/constraints.rs:95-116, prover2's components — as two expressions over the trace columns: the
 * multiplicity and relation.combine(values) = sum_i alpha^i values_i - z.  Those expressions, lowered like constraints (same opcodes,
 * loads of the component's preprocessed / main columns, any row offset) with one NX_C_FRAC / NX_C_FRACB per entry, ARE the
 * interaction trace: logup column j (batch j of finalize_logup / finalize_logup_in_pairs / finalize_logup_batched) holds the sum over
 * the entries of batches <= j of multiplicity / denominator — what the reference's hand-written generators (prover/src/traits.rs:
 * 124-145 -> every chip's fill_interaction_trace; prover2/machine/src/lookups/logup_trace_builder.rs:22-121) must compute too, or
 * their own constraints fail.  So the generator of EVERY chip and component moves to the device without touching one of them.
 * program: the fractions in non-decreasing batch order, every batch 0 .. n_logup_cols - 1 present; d_cols: the component's columns
 * as EVALUATIONS on the trace domain (bit-reversed circle-domain order, 2^log_size words; columns the program does not load may be
 * NULL — the interaction columns themselves always are); d_out: 4 n_logup_cols coordinate columns.  Follow with
 * nx_logup_finalize_last on the last column.  Compiled by hiprtc (cached per context; nx_air_cache_dir applies).
 * h_source_out (optional; then ctx / d_cols / d_out may be NULL and no GPU is needed): the generated HIP source. */
int nx_logup_program(nx_ctx* ctx, const nx_cinstr* program, uint32_t n_instr, uint32_t n_regs, const uint32_t* const* d_cols,
                     uint32_t n_cols, const uint32_t* econsts, uint32_t n_econsts, uint32_t log_size, uint32_t n_logup_cols,
                     uint32_t* const* d_out, char** h_source_out);

/* The TABLE side of a lookup: how often every table row was used, counted on the device.  The reference verifier refuses a proof
 * whose claimed sums do not cancel (prover/src/machine.rs:343; prover2/machine/src/verify.rs:145-160); they cancel only when the
 * table component's main-trace column holds the real counts.  The reference counts on the CPU, into the SideNote: the v1
 * Multiplicity<LEN, L> extensions (prover/src/extensions/multiplicity.rs:143-237), the bitwise tables, prover2's range_multiplicity /
 * bitwise_multiplicity components.  Here the looked-up columns are read where they are, in HBM.
 * uses: every place a tuple is looked up — n_key_cols device columns of 2^log_size canonical M31 words in ANY row order (bit-reversed
 * trace columns go in as they are) and the numerator column d_weight in the same order (NULL: every row counts 1; padding rows carry
 * 1 - is_padding).  At most 65536 uses, 2^30 rows per use and 2^32 rows in all per call (NX_ERR_ARG beyond: the sums stay below 2^63).
 * Key: the key columns are the tuple entries that determine the table row ([value] of a range table, (b, c) of a bitwise table); a
 * tuple (v_0 .. v_{k-1}) with v_i < 2^key_bits[i] has the key sum_i v_i << (key_bits[0] + .. + key_bits[i-1]).  1 <= n_key_cols <= 4,
 * 1 <= key_bits[i], sum of key_bits <= 24.  A lookup whose remaining entries disagree with the table is not seen here: its claimed
 * sums will not cancel.
 * d_table: n_key_cols device columns of 2^log_table words, the table component's preprocessed key columns as stored, in whatever order
 * they were committed (the reference's RangeValues holds value i at position i).  A table value outside its key_bits, or two table
 * rows with one key, is NX_ERR_ARG.
 * d_mult (device, 2^log_table words — typically the column nx_prover_tree_begin handed out for the table component, so nothing crosses
 * PCIe): d_mult[pos] = (sum of the weights of all rows of all uses whose key is the key of table row pos) mod p, canonical.  The sums
 * are exact 64-bit integers reduced once; only integer additions and minima are combined across lanes, so every run gives the same
 * words.
 * Missing rows: a row of nonzero weight (or of a use without weights) is missing when an entry is >= 2^key_bits[i] or no table row has
 * its key; rows of weight 0 never are.  n_missing / first_missing_use / first_missing_pos (each optional): their number and the smallest
 * (use index, storage position) among them.  With a missing row the call returns NX_ERR_PROTOCOL and nx_last_error names that row and
 * its values, "use 2 row position 17: (300) is not a row of the table"; d_mult is filled for the rows that are present.
 * Key spaces of up to 2^NX_MULT_LDS_MAX_KEY_BITS keys are counted in block-private LDS counters, wider ones with global atomics.
 * Blocking (it reports a count); temporaries (8 bytes per key of the key space) come from the context's allocator and are released
 * before it returns.  Every column may lie at any word-aligned address (a use whose columns are not all 16-byte aligned is read word by word). */
#define NX_MULT_LDS_MAX_KEY_BITS 12
typedef struct nx_lookup_use {
    const uint32_t* const* d_values;  /* n_key_cols device columns, 2^log_size canonical M31 words each, ANY row order */
    const uint32_t* d_weight;         /* NULL: every row counts 1; else a canonical M31 numerator column in the same row order */
    uint32_t log_size;
} nx_lookup_use;
int nx_logup_multiplicities(nx_ctx* ctx, const nx_lookup_use* uses, uint32_t n_uses, uint32_t n_key_cols, const uint32_t* key_bits,
                            const uint32_t* const* d_table, uint32_t log_table, uint32_t* d_mult, uint64_t* n_missing,
                            uint32_t* first_missing_use, uint64_t* first_missing_pos);

/* The same count for a table that is a SPARSE subset of a key space of up to 32 bits: the tables keyed by an address.  prover2's
 * PrivateMemoryBoundary has one row per touched RAM address, with MultiplicityRead / MultiplicityWrite from the AddressAccessSideNote
 * (prover2/machine/src/components/read_write_memory_boundary/private_memory/mod.rs:95-168, consumed at :249-262;
 * read_write_memory/trace.rs:70-71,122,218); its Pub / Static / ProgramMemoryBoundary (keyed by pc) and v1's FinalPrgMemoryCtr are
 * keyed the same way.  nx_logup_multiplicities would need a counter per key of the key space, 32 GiB for such a table; here the
 * counters belong to the table's rows and a looked-up row finds its counter by a search.
 * Everything is as in nx_logup_multiplicities — the uses (any row order, optional d_weight, at most 65536 uses, 2^30 rows per use,
 * 2^32 rows in all), exact 64-bit sums reduced once mod p, the rule for missing rows and the text that names the first one,
 * NX_ERR_PROTOCOL with d_mult still filled for the rows that are present, the same words on every run, blocking, every column at any
 * word-aligned address — except:
 * Key: 1 <= n_key_cols <= 4, 1 <= key_bits[i] <= 32, sum of key_bits <= 32; the packed key is that of nx_trace_prev_access.
 * Table rows: d_table_valid is NULL (every row is a table row) or a column of 2^log_table words; a row is a table row iff its word is
 * nonzero (the complement of IsPad).  The other rows may hold anything, copies of valid keys and values outside their bits included;
 * d_mult gets 0 there, so every word of d_mult is written.  0 <= log_table <= 30.  A table without any valid row is legal: every row
 * of nonzero weight is then missing.
 * NX_ERR_ARG (nothing stays allocated, the context stays usable): the pointer and count refusals of nx_logup_multiplicities; d_mult
 * equal to any input column pointer of the call; a valid table row with an entry >= 2^key_bits[i] ("table row position 5 holds a
 * value outside its key_bits"); two valid table rows with one key — nx_last_error names the smallest position whose key also lies at
 * a smaller valid position, that smallest position and the entries ("table row positions 3 and 9 hold the same key (7, 65535)").
 * How: the valid rows become (key, position) pairs sorted by key (ceil(sum of key_bits / 8) stable counting passes); a row of a use
 * finds its key by a binary search whose upper level — every 2^(log_table - NX_MULT_SPARSE_LDS_LOG_KEYS)-th sorted key — is staged
 * in LDS; a table of up to 2^NX_MULT_SPARSE_LDS_LOG_KEYS rows is searched in LDS alone.
 * DEVICE MEMORY: with T = 2^log_table and U = n_uses,
 *     peak above the caller's columns  <=  16 T + 1024 min(256, ceil(T / 1024)) + 52 U + 4 * 2^NX_MULT_SPARSE_LDS_LOG_KEYS + 4096 bytes
 * (two (key, position) buffers of 8 T each, of which the one the last sort pass has read then holds the 64-bit counters; the per-block
 * digit counts of a pass; the use table; the splitters of a table the LDS does not hold whole) and NOTHING per key of the key space.  Taken from the context's allocator, released before
 * the call returns. */
#ifndef NX_MULT_SPARSE_LDS_LOG_KEYS
#define NX_MULT_SPARSE_LDS_LOG_KEYS 12
#endif
int nx_logup_multiplicities_sparse(nx_ctx* ctx, const nx_lookup_use* uses, uint32_t n_uses, uint32_t n_key_cols, const uint32_t* key_bits,
                                   const uint32_t* const* d_table, const uint32_t* d_table_valid, uint32_t log_table, uint32_t* d_mult,
                                   uint64_t* n_missing, uint32_t* first_missing_use, uint64_t* first_missing_pos);

/* ------------------------------------------- memory-checking columns: what the PREVIOUS access to the same address left behind ----
 * The reference fills these in one sequential pass over a map: Reg{1,2,3}TsPrev / ValPrev from RegisterMemCheckSideNote::access
 * (prover/src/chips/memory_check/register_mem_check.rs:53-118,401-425; prover/src/trace/regs.rs:29-37), Ram{1..4}TsPrev / ValPrev from
 * ReadWriteMemCheckSideNote::last_access (prover/src/chips/instructions/i/load_store.rs:180-221; prover/src/trace/sidenote/mod.rs:
 * 25-47), ProgCtrPrev from last_access_counter (prover/src/chips/memory_check/program_mem_check.rs:49-96), and from what the map holds
 * at the end the rows of the final-state tables (FinalPrgMemoryCtr, extensions/final_reg.rs, extensions/ram_init_final.rs).  They are
 * not row-local, so nx_trace_program refuses them.  Here every access of every stream becomes one element (packed key, handle),
 * enumerated in time order; a stable LSD radix sort by the key (8-bit digits) then puts every access next to its predecessor, the
 * first access of a key at the head of its run and the last one at its tail.
 * TIME ORDER (total): lexicographic in (epoch, natural trace row, index of the stream in `streams`).  The natural row of a stream with
 * linear == 0 is the coset-order row of the storage position (columns in bit-reversed circle-domain order, the rule of nx_air_check,
 * nx_logup_program and nx_trace_program); with linear != 0 it is the position itself (a memory image).  Registers: three streams of
 * one epoch in slot order.  RAM: the initial image as a linear stream of epoch 0 with d_prev == NULL, the four byte streams of the
 * load/store chip with epoch 1.  Streams may have different log_size (1..30; 0..30 when linear; fewer than 2^31 rows in all, at most
 * 65536 streams).
 * KEY: as in nx_logup_multiplicities, entry i < 2^key_bits[i], the packed key is sum_i entry_i << (key_bits[0] + .. + key_bits[i-1]);
 * 1 <= n_key_cols <= 4, 1 <= key_bits[i], sum of key_bits <= 32.
 * For a row that accesses (d_flag == NULL or its word != 0): d_prev[c][pos] = payload column c of the latest earlier access with the
 * same key, from whichever stream (0 where that stream's d_payload[c] is NULL), or init[c] when there is none; d_ordinal[pos] = the
 * number of earlier accesses to the key.  For a row that does not access: every d_prev column and d_ordinal get 0 at its position —
 * the outputs are fully defined, no memset is needed.  1 <= n_payload <= 16; init: n_payload canonical words, NULL = all 0.
 * summary (optional): one entry per distinct key in ascending order of the packed key — the key, the number of accesses to it and the
 * payload of its LAST access; the first min(cap, number of keys) entries are written (entries of d_last may be NULL).  *n_keys
 * (optional) always receives the number of distinct keys; more keys than cap is not an error.
 * Exact and order-free: only integers are compared, counted and copied, every word is the same on every run.
 * NX_ERR_ARG (nx_last_error names the argument; nothing is launched): a NULL ctx, streams, key_bits or key column; n_streams of 0 or
 * above 65536; n_payload of 0 or above 16; bad key_bits; an init word >= p; a log_size outside its range; 2^31 rows or more in all;
 * an output pointer (d_prev entry, d_ordinal, summary array) equal to any other column pointer of the call.  A stream that asks for no
 * output is fine.  NX_ERR_PROTOCOL: an accessing row holds a key entry >= 2^key_bits[i]; nx_last_error names the smallest (stream,
 * storage position) and the value ("stream 2 row position 17: key entry 0 holds 300, outside its 8 bits"); the outputs are then
 * unspecified, the context stays usable.
 * DEVICE MEMORY: with A = the rows of all streams (every row is an element of the sort, accessing or not) and S = n_streams,
 *     peak above the caller's columns  <=  18 A + 1024 S + 65536 bytes
 * (two (key, handle) buffers of 8 A each, the per-block digit counts, A at most and never above 1 MiB, A / 128 for the run heads) and NOTHING per
 * distinct key: the summary goes straight into the caller's arrays.  Taken from the context's allocator, released before the call
 * returns.  Blocking.  ceil(sum of key_bits / 8) sort passes, one more when some stream has a d_flag and the sum is a multiple of 8
 * (rows that do not access sort behind the largest key).  Every column may lie at any word-aligned address (a stream whose columns are not
 * all 16-byte aligned is read and written word by word). */
typedef struct nx_access_stream {
    const uint32_t* const* d_key;      /* n_key_cols columns, 2^log_size canonical words                      */
    const uint32_t* d_flag;            /* NULL: every row is an access; else the row accesses iff word != 0   */
    const uint32_t* const* d_payload;  /* n_payload columns: what this access leaves behind (current          */
                                       /* timestamp limbs, current value limbs ...); an entry may be NULL = 0 */
    uint32_t* const* d_prev;           /* NULL, or n_payload output columns (an entry may be NULL: not wanted) */
    uint32_t* d_ordinal;               /* NULL, or output: number of earlier accesses to the same key         */
    uint32_t log_size, epoch, linear;  /* linear != 0: position == row; else bit-reversed circle-domain order */
} nx_access_stream;
typedef struct nx_access_summary {     /* optional: one entry per distinct key, ascending packed key           */
    uint32_t cap;                      /* capacity of the arrays below                                         */
    uint32_t* d_key;                   /* packed key                                                           */
    uint32_t* d_count;                 /* accesses to it (FinalPrgMemoryCtr)                                   */
    uint32_t* const* d_last;           /* n_payload columns: payload of its LAST access (final ts / value)     */
} nx_access_summary;
int nx_trace_prev_access(nx_ctx* ctx, const nx_access_stream* streams, uint32_t n_streams, uint32_t n_key_cols,
                         const uint32_t* key_bits, uint32_t n_payload, const uint32_t* init, const nx_access_summary* summary,
                         uint64_t* n_keys);

/* ------------------------------------------- memory-checking columns when an access leaves behind what depends on what it FOUND ---
 * nx_trace_prev_access needs every access to know in advance what it leaves.  The load/store chip does (last_access.insert(addr,
 * (clk, value)), prover/src/chips/instructions/i/load_store.rs:199-205); the keccak chip does not: KeccakChip::update_state_timestamps
 * (prover/src/chips/custom.rs:107-123) touches the 200 bytes at addr + i, reports the timestamp it finds and leaves ts + 1 with the
 * output byte, so two calls on one buffer chain through each other and every later load or store of those bytes reads the chained
 * value as Ram*TsPrev.  This entry is nx_trace_prev_access with two additions: payload columns may CHAIN, and a stream may be a list
 * of BLOCK records.  It is the stage between nx_trace_keccak_round (whose d_states_out it reads as bytes) and
 * nx_trace_keccak_memory_check (whose d_timestamps it writes).
 * A COLUMN stream (d_row == NULL) is an nx_access_stream: one access per position of 2^log_size; its natural row is the coset-order
 * row of the position, or the position itself when linear != 0.  A BLOCK stream (d_row != NULL) is a list of n_records records, the
 * keccak instances: record j makes `span` accesses at natural row d_row[j], sub-access i to the packed key key(j) + i, where key(j) is
 * packed from d_key[k][j].  d_key[k], d_flag and d_row hold one word per record; every per-access array of a block stream is
 * record-major, element j * span + i: d_payload[c] of a GIVEN column one word per element, or with NX_CHAIN_BYTES byte i of a record of
 * `span` bytes (records contiguous, the array 4-byte aligned, span % 4 == 0: the layout of d_states_out); d_prev[c] and d_ordinal one
 * word per element (the layout nx_trace_keccak_memory_check reads as d_timestamps).  log_size is ignored for a block stream, n_records
 * and span for a column stream.  At most 8 block streams per call; 1 <= span <= 256; n_records may be 0.
 * TIME ORDER (total): lexicographic in (epoch, natural row, index of the stream in `streams`, sub-access i).
 * CHAINING: walk the accesses to one key in time order with a state of n_payload words that starts at init.  An access gets the state
 * as d_prev and the number of earlier accesses to the key as d_ordinal; then every word c is replaced by the access's payload
 * (rule[c] NX_CHAIN_GIVEN: d_payload[c] at its element, 0 where that pointer is NULL) or has delta[c] added to it modulo 2^32
 * (NX_CHAIN_ADD; d_payload[c] must be NULL).  rule and delta belong to the stream: a column may be ADD in one stream and GIVEN in
 * another.  The summary's d_last[c] is the state after the last access to the key, whatever the rules.  Words are raw 32-bit integers:
 * nothing in device memory is validated for canonicity (as nx_trace_keccak_memory_check); only init must be below p.
 * Rows and records that do not access (d_flag word == 0) get 0 in every output word of theirs; every output word is written.
 * With no block stream and every rule GIVEN each output word equals nx_trace_prev_access's on the same streams.
 * Exact and order-free: only integers are compared, counted, added and copied; every run gives the same words.  Blocks meet at kernel
 * boundaries only.
 * NX_ERR_ARG (nx_last_error names the argument; nothing is launched, nothing stays allocated): everything nx_trace_prev_access
 * refuses (for column streams: log_size; 2^31 ELEMENTS or more in all, an element being a row of a column stream or one of the
 * n_records * span accesses of a block stream); a span of 0 or above 256; more than 8 block streams; NX_CHAIN_BYTES on a column
 * stream, on an ADD column, with span % 4 != 0 or with a payload pointer that is not 4-byte aligned; an ADD column with a non-NULL
 * d_payload[c]; a rule word that is none of these.
 * NX_ERR_PROTOCOL (outputs unspecified, the context stays usable; nx_last_error names the smallest offender by stream, then storage
 * position or record, then sub-access): an accessing row or record with a key entry >= 2^key_bits[i] ("stream 2 record 3: key entry 0
 * holds 300, outside its 8 bits"); a sub-access key at or above 2^(sum of key_bits) ("stream 1 record 4 sub-access 7: key 4294967290
 * + 7 is outside the 32 key bits"); a d_row that is not strictly ascending, named at the first record whose row is not above its
 * predecessor's ("stream 1 record 2: d_row of 5 is not above its predecessor's 9"), or not below 2^31.  These are read back before
 * anything is sorted.
 * DEVICE MEMORY: with A = the elements of all streams (accessing or not) and S = n_streams,
 *     peak above the caller's columns  <=  18 A + 1024 S + 65536 bytes
 * (two (key, handle) buffers of 8 A each; the per-block digit counts, A at most and never above 1 MiB; per 1024 sorted elements the
 * head count, the last head and two words per chained column) and NOTHING per distinct key.  Taken from the context's allocator,
 * released before the call returns.  Blocking.  Sort passes as nx_trace_prev_access.  Every column may lie at any word-aligned
 * address. */
#define NX_CHAIN_GIVEN 0u  /* the access leaves d_payload[c] behind (NULL pointer: 0): the rule of nx_trace_prev_access           */
#define NX_CHAIN_ADD   1u  /* the access leaves (what it found + delta[c]) mod 2^32 behind; d_payload[c] must be NULL              */
#define NX_CHAIN_BYTES 2u  /* ORed to GIVEN, block streams only: d_payload[c] holds `span` BYTES per record                        */
typedef struct nx_chain_stream {
    const uint32_t* const* d_key;      /* n_key_cols columns: the key of sub-access 0                                  */
    const uint32_t* d_flag;            /* NULL: every row / record accesses                                            */
    const uint32_t* d_row;             /* NULL: a COLUMN stream (as nx_access_stream).  Else a BLOCK stream: n_records  */
                                       /* words, strictly ascending natural rows < 2^31; record j happens at d_row[j]  */
    const uint32_t* const* d_payload;  /* n_payload entries                                                            */
    const uint32_t* rule;              /* n_payload words (host), NULL = all NX_CHAIN_GIVEN                            */
    const uint32_t* delta;             /* n_payload words (host, read for ADD columns), NULL = all 1                   */
    uint32_t* const* d_prev;           /* NULL, or n_payload outputs (entries may be NULL)                             */
    uint32_t* d_ordinal;               /* NULL, or output                                                              */
    uint32_t log_size;                 /* column stream                                                                */
    uint32_t n_records, span;          /* block stream: 0 <= n_records, 1 <= span <= 256                               */
    uint32_t epoch, linear;
} nx_chain_stream;
int nx_trace_access_chain(nx_ctx* ctx, const nx_chain_stream* streams, uint32_t n_streams, uint32_t n_key_cols,
                          const uint32_t* key_bits, uint32_t n_payload, const uint32_t* init, const nx_access_summary* summary,
                          uint64_t* n_keys);

/* ------------------------------------------- derived trace columns filled on the device from a recorded ROW PROGRAM --------------
 * The reference fills the main trace on the CPU: MachineChip::fill_main_trace (prover/src/traits.rs:34-40) runs every chip on every
 * row, and almost every chip is a row-local integer function of a few seed columns — AddChip's ValueA bytes and CarryFlag bits from
 * ValueB / ValueC (prover/src/chips/instructions/i/add.rs:26-96), SllChip's Rem / Qt / shift bits (sll.rs:33-111), the range, bit-op,
 * compare and branch chips; the preprocessed is_first and counter columns depend on the row number only (prover/src/trace/
 * preprocessed.rs:65-99).  A host that uploads the seed columns and derives the rest here moves a fraction of the trace over PCIe.
 * A trace program is an nx_cinstr array over the BASE-FIELD register file: NX_C_LOAD (row offset taken in natural trace order, row
 * (i + o) mod 2^log_size, the rule of nx_air_check and nx_logup_program), NX_C_CONST, NX_C_ADD, NX_C_SUB, NX_C_MUL, NX_C_NEG and the
 * opcodes below.  Registers always hold canonical words: the 32-bit integer result r of an integer opcode is written as r mod p (only
 * OR, XOR and SHL can reach p), so there is no error path at run time.  A second register kind, W, holds a raw 32-bit integer
 * (NX_T_PACK32 .. NX_T_REMU32): PACK32 makes one from two half-words, MULLO32 / MULHU32 / DIVU32 / REMU32 work on them with RISC-V's
 * total division, LO16 / HI16 take the halves back into canonical words.  Signed MULH / DIV / REM need no opcode: the chips work on
 * absolute values, signs and borrows, which the existing opcodes give. */
enum {
    NX_T_STORE = 32,    /* cols[a][row] = B[b]                                   (dst must be 0)                       */
    NX_T_STORE_IF = 33, /* if (B[dst] != 0) cols[a][row] = B[b]; the column keeps its content elsewhere: several chips  */
                        /* share one column (ValueA), each on the rows of its own opcode flag                           */
    NX_T_ROW = 34,      /* B[dst] = the natural trace row i (the VM step), not the storage position                     */
    NX_T_AND = 35, NX_T_OR = 36, NX_T_XOR = 37, /* B[dst] = B[a] op B[b], the canonical words as 32-bit integers        */
    NX_T_SHL = 38,      /* B[dst] = (B[a] << B[b]) truncated to 32 bits; a count >= 32 gives 0                          */
    NX_T_SHR = 39,      /* B[dst] = B[a] >> B[b]; a count >= 32 gives 0                                                 */
    NX_T_LTU = 40, NX_T_EQ = 41, /* B[dst] = 1 if B[a] < B[b] / B[a] == B[b] as integers, else 0                        */
    NX_T_INV = 42,      /* B[dst] = the M31 inverse of B[a]; the inverse of 0 is 0 (is-zero helper columns)             */
    /* The W kind: one register holding a raw 32-bit integer that need not be canonical (the RV32M chips' 64-bit product bytes and
     * quotients: prover/src/chips/instructions/m/).  A register has the kind its latest writer gave it; the program is straight-line,
     * so the kind at every instruction is static.  Every opcode is a total function.                                              */
    NX_T_PACK32 = 43,   /* W[dst] = (B[a] + (B[b] << 16)) truncated to 32 bits: a low and a high half-word                   */
    NX_T_LO16 = 44,     /* B[dst] = W[a] & 0xFFFF                                  (b must be 0)                       */
    NX_T_HI16 = 45,     /* B[dst] = W[a] >> 16                                     (b must be 0)                       */
    NX_T_MULLO32 = 46,  /* W[dst] = the low 32 bits of W[a] * W[b]                                                      */
    NX_T_MULHU32 = 47,  /* W[dst] = the high 32 bits of the unsigned 64-bit product W[a] * W[b]                         */
    NX_T_DIVU32 = 48,   /* W[dst] = W[a] / W[b] unsigned; W[b] == 0 gives 0xFFFFFFFF (RISC-V DIVU)                      */
    NX_T_REMU32 = 49    /* W[dst] = W[a] % W[b] unsigned; W[b] == 0 gives W[a]       (RISC-V REMU)                      */
};
/* Runs the program once per row and stores into d_cols, TRACE-DOMAIN EVALUATIONS in bit-reversed circle-domain order, 2^log_size
 * words each (1 <= log_size <= 30) — what nx_prover_tree_begin hands out before the commit; preprocessed, main and scratch columns
 * may be mixed in one table, entries the program neither loads nor stores may be NULL.  One work-item per storage position (it
 * derives its natural row once), stores go to the lane's own position; a program whose loads all have offset 0 (the row-local chips)
 * runs with four consecutive positions per lane and 16-byte loads and stores when every column it touches is 16-byte aligned and the
 * trace has at least four rows (context option "trace.vec4"; the same words either way).  A program too large for the instruction cache is cut at
 * store boundaries into kernels of at most "air.segment" estimated instructions, launched one after the other.
 * Refused with NX_ERR_ARG (nx_last_error names the instruction): a secure-field, constraint or fraction opcode; a program without a
 * store; a register read before an earlier instruction wrote it; a 32-bit integer opcode whose operand register is not W at that
 * point; any other opcode (STORE and the STORE_IF flag included) reading a register that is W at that point; a nonzero b on LO16 /
 * HI16; an opcode of 50 or more; a LOAD, at any offset, of a column that some store of the program
 * targets (lanes would race: chain two calls instead); a loaded or stored column whose pointer is NULL; an output column whose
 * pointer equals that of another entry of d_cols; a register out of range, a column index >= n_cols, an immediate >= p.
 * Stream-ordered like nx_air_eval: validation errors are returned at once, a later commit, check or download orders after the
 * launch.  Compiled by hiprtc on first use and kept per context, keyed by the program bytes (nx_air_cache_dir and the helper-process
 * compilation apply; released by nx_ctx_destroy).  No device memory is allocated: the pointer table travels through the context's
 * staging ring.  h_source_out (optional; when it is the only output wanted ctx and d_cols may be NULL and no GPU is needed): the
 * generated HIP source (free with nx_free_host). */
int nx_trace_program(nx_ctx* ctx, const nx_cinstr* program, uint32_t n_instr, uint32_t n_regs, uint32_t* const* d_cols,
                     uint32_t n_cols, uint32_t log_size, char** h_source_out);

/* ------------------------------------------- the keccak round trace filled on the device from the instances' input states --------
 * The reference's KeccakRound component (prover/src/extensions/keccak/round/trace.rs:240-366) is its widest trace: 1705 main columns,
 * every intermediate 64-bit lane of one keccak-f[1600] round as 8 byte columns.  Row i of an instance holds the state after i rounds,
 * so the 200 seed columns are not row-local and nx_trace_program cannot fill them; the device needs the 200 bytes of an instance, not
 * 6.8 KB per row.
 * d_states: n_instances x 25 little-endian 64-bit lanes in device memory, lane (x, y) at index x + 5 y (KeccakSideNote::inputs); may be
 * NULL when n_instances == 0.  With rounds = 2^log_rounds, natural trace row r = instance * rounds + i holds the round with constant
 * RC[first_round + i] applied to the instance's state after i earlier rounds of the component.  Rows r >= n_instances * rounds are
 * padding: their input state is zero and every derived column follows from it (the iota output is the round-constant bytes, the rest
 * 0); is_padding is 1 on them.
 * d_main: NX_KECCAK_ROUND_MAIN_COLS device columns of 2^log_size words, TRACE-DOMAIN EVALUATIONS in bit-reversed circle-domain order
 * (what nx_prover_tree_begin hands out; the rule of nx_trace_program), in the order the reference's builder allocates them, every lane
 * as 8 byte columns, low byte first: the 25 input lanes; theta: the 4 chained xors of each of the 5 columns; for each x low / high /
 * out of rot(C[x+1], 1), then D[x]; the 25 A ^ D lanes, x outer and y inner; rho-pi: low / high / out of each of the 24 nonzero
 * rotations in (x, y) loop order; chi: not-and, then xor, per (x, y); iota: A[0] ^ RC; is_padding.  A rotation by r has
 * low = (byte << (r % 8)) & 255, high = byte >> (8 - r % 8) and out byte i = low[(i - r/8) & 7] + high[(i - r/8 + 7) & 7]; rotations
 * by 8 and 56 still have their three lanes (high = 0).
 * d_pre: NULL, or NX_KECCAK_ROUND_PRE_COLS columns: the 8 bytes of RC[first_round + (r mod rounds)] on EVERY row, padding included,
 * then is_last: 1 at natural row 2^log_size - 1, else 0.
 * d_states_out: NULL, or n_instances x 25 lanes: the state after the component's last round (the reference's `rem`), the next
 * component's d_states.
 * Exact integers: the same words on every run.  One work-item per storage position.  Stream-ordered like nx_trace_program; no device
 * memory is allocated, the pointer table travels through the context's staging ring.
 * NX_ERR_ARG (nx_last_error names the argument; nothing is launched): first_round + 2^log_rounds > 24; log_size outside 1..30;
 * n_instances * rounds > 2^log_size; a NULL or repeated column pointer, a pointer shared between d_main and d_pre; d_states NULL with
 * n_instances > 0; d_states or d_states_out not 8-byte aligned; d_states_out overlapping d_states (lanes of one instance would race);
 * a NULL ctx. */
#define NX_KECCAK_ROUND_MAIN_COLS 1705   /* 213 byte-limb lanes of 8 columns + is_padding */
#define NX_KECCAK_ROUND_PRE_COLS  9      /* 8 round-constant byte columns + is_last */
int nx_trace_keccak_round(nx_ctx* ctx, const uint64_t* d_states, uint32_t n_instances, uint32_t first_round, uint32_t log_rounds,
                          uint32_t log_size, uint32_t* const* d_main, uint32_t* const* d_pre, uint64_t* d_states_out);

/* ------------------------------------------- the keccak memory-check trace filled on the device from the instances' inputs ----------
 * The reference's PermutationMemoryCheck component (prover/src/extensions/keccak/memory_check/trace.rs:32-123) hands the input state to
 * the first KeccakRound component, takes the output state back from the second and charges the 200 byte accesses of every call to the
 * load/store memory argument: 2001 main columns, computed on the CPU with a full keccakf per row.  The device needs the 1004 bytes of
 * an instance: its state, one address and 200 timestamps.
 * d_states: n_instances x 25 little-endian 64-bit lanes (the first round component's d_states); d_addresses: n_instances words
 * (KeccakSideNote::addresses); d_timestamps: n_instances x 200 words, instance-major (KeccakSideNote::timestamps[row][byte]), 16-byte
 * aligned (a work-item reads its 800 bytes as 16-byte loads).  Each may be NULL when n_instances == 0.  Natural trace row r is instance
 * r.  Rows r >= n_instances are padding: every column is 0 on them except is_padding, which is 1 (out_state too: it is NOT keccak-f of
 * the zero state, trace.rs:41 writes the real rows only).
 * d_main: NX_KECCAK_MEMCHECK_MAIN_COLS device columns of 2^log_size words, TRACE-DOMAIN EVALUATIONS in bit-reversed circle-domain order
 * (the rule of nx_trace_keccak_round), in the order of trace.rs:34: the 200 input-state bytes (lane l, byte b at 8 l + b); the 200
 * output-state bytes, keccak-f[1600] of the input; 400 address limbs, for i in 0..200 the low 16 bits of addr + i, then the high 16;
 * 400 previous-timestamp limbs, low then high of ts[i]; 400 next-timestamp limbs, of ts[i] + 1; 200 address carries,
 * ((addr + i) & 0xFFFF) == 0xFFFF; 200 timestamp carries, (ts[i] & 0xFFFF) == 0xFFFF; is_padding.
 * addr + i and ts[i] + 1 are taken MODULO 2^32: an address above 2^32 - 200 or a timestamp of 2^32 - 1 gives columns that do not
 * satisfy the component's constraints, and nx_prover_check names the row; the call validates nothing that lies in device memory.
 * d_pre: NULL, or NX_KECCAK_MEMCHECK_PRE_COLS column: is_last, 1 at natural row 2^log_size - 1, else 0.
 * d_states_out: NULL, or n_instances x 25 lanes: the permuted states, equal to the second round component's d_states_out.
 * Exact integers: the same words on every run.  One work-item per storage position.  Stream-ordered like nx_trace_keccak_round; no
 * device memory is allocated, the pointer table travels through the context's staging ring.
 * NX_ERR_ARG (nx_last_error names the argument; nothing is launched): log_size outside 1..30; n_instances > 2^log_size; a NULL or
 * repeated column pointer, a pointer shared between d_main and d_pre; d_states, d_addresses or d_timestamps NULL with n_instances > 0;
 * d_states or d_states_out not 8-byte aligned; d_timestamps not 16-byte aligned; d_states_out overlapping d_states; a NULL ctx. */
#define NX_KECCAK_MEMCHECK_MAIN_COLS 2001   /* 2 x 200 state bytes, 3 x 400 limbs, 2 x 200 carries, is_padding */
#define NX_KECCAK_MEMCHECK_PRE_COLS  1      /* is_last */
int nx_trace_keccak_memory_check(nx_ctx* ctx, const uint64_t* d_states, const uint32_t* d_addresses, const uint32_t* d_timestamps,
                                 uint32_t n_instances, uint32_t log_size, uint32_t* const* d_main, uint32_t* const* d_pre,
                                 uint64_t* d_states_out);

/* ------------------------------------------- the step table split into per-opcode component traces on the device ------------------
 * Every execution component of the reference's v2 prover takes the steps of its own opcode only: ExecutionComponent::iter_program_steps
 * (prover2/machine/src/components/execution/common/mod.rs:31-39) filters the whole execution by OPCODE, row i of the component is the
 * i-th such step, and the trace is padded to 2^max(ceil_log2(count), LOG_N_LANES) rows with IsLocalPad = 1 (execution/add/mod.rs:
 * 157-183; the same in sub, sll, load, store ...); the Cpu component takes every step (components/cpu/trace.rs:36-59).  The four device
 * fills above want a component's seed columns in device memory, one row per step OF THAT COMPONENT; these two calls make them from ONE
 * step table, so an execution crosses PCIe once, as 32-bit words.
 * STEP TABLE: n_src device columns of n_steps words in step order — linear, NOT bit-reversed; 0 <= n_steps <= 2^30 (pc, clk, instr,
 * operand values, a result ...).  CLASS COLUMN d_class: n_steps words, the component of each step, 0 .. n_classes - 1, or NX_PART_NONE
 * for a step that belongs to no component; 1 <= n_classes <= NX_PART_MAX_CLASSES.
 * nx_trace_partition_create counts the steps of every class into counts[n_classes] (host memory; blocking, like the other calls that
 * report a count) and keeps the STABLE ORDER — for class c the steps with d_class == c in execution order — in *out: one index array
 * of n_steps words from the context's allocator, released by nx_trace_partition_destroy (NULL is fine), and n_classes + 1 offsets in
 * host memory; nothing else stays on the device.  One 8-bit counting pass: per-block class histogram, scan, stable placement.  d_class
 * is read again by no later call, but nx_trace_partition_fill compares its pointer with the outputs.
 * nx_trace_partition_log_size(count, min_log) = max(ceil_log2(count), min_log), count 0 giving min_log: the component's log_size for
 * nx_prover_tree_begin.  Pure host arithmetic.
 * nx_trace_partition_fill makes n_dests components in one call.  A destination has a class (NX_PART_ALL: every step in step order,
 * the Cpu component), a log_size in 1..30 with 2^log_size >= the class's count, n_cols output columns of 2^log_size words — TRACE-
 * DOMAIN EVALUATIONS in bit-reversed circle-domain order, the rule of nx_trace_program — and one limb spec {src, shift, bits} per
 * output column: natural row r < count holds (d_src[src][step_r] >> shift) & (2^bits - 1), step_r the r-th step of the class;
 * 1 <= bits <= 31, shift + bits <= 32; the value p is written as 0 (nx_trace_program's rule for integer results).  Rows r >= count
 * hold 0.  d_is_pad (optional): 0 on real rows, 1 on padding rows (IsLocalPad / IsPad); d_step (optional): the step index of the row,
 * 0 on padding rows.  EVERY word of every output is written: no memset is needed.  The reference's fill_columns(row, pc_parts,
 * Column::Pc) and fill_columns_bytes(row, &value_b, Column::BVal) become limb specs over one word column; derived columns (PcCarry,
 * ClkCarry, AVal, HCarry ...) stay with nx_trace_program on the component's own columns.  Several destinations may have one class.  A
 * source word is loaded once per row however many limbs are cut from it.  Stream-ordered like nx_trace_program; no device memory is
 * allocated by the fill, the descriptor tables travel through the context's staging ring.
 * Exact integers: the same words on every run.
 * NX_ERR_ARG (nx_last_error names the argument; nothing is launched): a NULL ctx, out, counts or partition; d_class NULL with
 * n_steps > 0; n_classes of 0 or above 256; n_steps above 2^30; a context that is not the partition's; a destination whose class is
 * >= n_classes and not NX_PART_ALL; a log_size outside 1..30 or with 2^log_size < count; src >= n_src; bad shift / bits; a NULL
 * output column, or a NULL d_src entry that a spec names when n_steps > 0; an output pointer (column, d_is_pad, d_step) equal to
 * another output of the call or to a source or class column.
 * NX_ERR_PROTOCOL (create): a class word >= n_classes that is not NX_PART_NONE; nx_last_error names the SMALLEST such step and its
 * word, "step 17: class 300, 40 classes"; *out is NULL, the context stays usable and its live bytes are what they were.
 * n_steps == 0 is valid: every count is 0, every destination row is padding.
 * DEVICE MEMORY: create keeps 4 n_steps bytes (the order) and needs, until it returns, 4 n_classes B + 1280 bytes more, B <= 1024
 * the blocks of the counting pass (each term rounded up to 256). */
#define NX_PART_NONE 0xFFFFFFFFu       /* class word of a step that belongs to no component */
#define NX_PART_ALL  0xFFFFFFFFu       /* class of a destination that takes every step in step order */
#define NX_PART_MAX_CLASSES 256
typedef struct nx_partition nx_partition;
typedef struct nx_part_limb { uint32_t src, shift, bits; } nx_part_limb;
typedef struct nx_part_dest {
    uint32_t cls;                      /* 0 .. n_classes - 1, or NX_PART_ALL                                  */
    uint32_t log_size;                 /* 1 .. 30, 2^log_size >= the steps of the class                       */
    uint32_t n_cols;
    uint32_t* const* d_cols;           /* n_cols output columns of 2^log_size words                           */
    const nx_part_limb* limbs;         /* n_cols specs, one per output column                                 */
    uint32_t* d_is_pad;                /* NULL, or output: 0 on real rows, 1 on padding rows                  */
    uint32_t* d_step;                  /* NULL, or output: the step index of the row, 0 on padding rows       */
} nx_part_dest;
int nx_trace_partition_create(nx_ctx* ctx, const uint32_t* d_class, uint32_t n_steps, uint32_t n_classes, uint32_t* counts,
                              nx_partition** out);
uint32_t nx_trace_partition_log_size(uint64_t count, uint32_t min_log);
int nx_trace_partition_fill(nx_ctx* ctx, const nx_partition* part, const uint32_t* const* d_src, uint32_t n_src,
                            const nx_part_dest* dests, uint32_t n_dests);
void nx_trace_partition_destroy(nx_partition* part);

/* Config #2: LDE + Blake2s commit of n_cols random columns of 2^log_size rows (already resident,
 * bit-reversed evaluations, overwritten by their coefficients); d_lde receives the LDE columns. */
int nx_lde_commit(nx_ctx* ctx, const nx_twiddles* tw, uint32_t* const* d_cols, uint32_t n_cols, uint32_t log_size,
                  uint32_t log_blowup, uint32_t* const* d_lde, uint8_t root[32]);

/* The ROOT of that commitment without keeping the extension or the tree — what a verifier needs of the preprocessed columns: the
 * reference re-commits them at full height in every verification only to compare 32 bytes (prover/src/machine.rs:363-417,
 * prover2/machine/src/verify.rs:103-143).  d_cols: n_cols columns in commit order, column i of 2^log_sizes[i] words
 * (trace sizes, mixed sizes allowed; bit-reversed evaluations on entry, CONSUMED like nx_lde_commit's: they hold the coefficients on
 * return).  The columns of the largest size are extended in chunks of C = 16 (one Blake2s block of the leaf chain) into a ring of R = 2
 * slots and absorbed by the leaf chain while the next chunk transforms; no extension outlives its chunk.  The inner layers are reduced
 * to the root three levels per launch between two buffers, none of them stored.  Same root as nx_lde_commit / nx_prover_tree_commit of
 * the same columns, for both node-hash rules; n_cols = 0 gives the root of the empty tree.
 * DEVICE MEMORY: with M = 2^(max log_size + log_blowup) rows, n the number of columns of the largest size and S the smaller columns,
 *     peak above the inputs  <=  4 M min(C, n) min(R, ceil(n / C))      the ring
 *                              + 32 M                                    the running leaf state
 *                              + 32 M / 2^k                              the second reduction buffer; k = 3 when all columns have one size,
 *                                                                        else min(3, max(1, d - 1)) with 2^d = largest size / next smaller size
 *                              + sum over S of 4 * 2^(log_size + log_blowup)   smaller columns, kept whole until their layer is hashed
 * bytes, each term rounded up to 256 — independent of n beyond the ring.  (nx_lde_commit: 4 M n for the extensions plus 64 M for the tree.)
 * Blocking (returns the root). */
int nx_commit_root(nx_ctx* ctx, const nx_twiddles* tw, uint32_t* const* d_cols, const uint32_t* log_sizes, uint32_t n_cols,
                   uint32_t log_blowup, uint8_t root[32]);

#ifdef __cplusplus
}
#endif
#endif /* NEXUS_HIP_H */
