"""The failure side of tests/poison_sites.py: for every place under csrc/ that takes a block from the context's caching allocator, who
gives back the blocks taken EARLIER in the same function when THIS request is refused (NX_ERR_OOM from the driver, from the context
option "mem.limit_bytes" or from "debug.fail_alloc"), and what the caller of the function sees.  The contract the rows add up to is in
the context section of include/nexus_hip.h ("AFTER NX_ERR_OOM").  Rows cite functions and types by name, never by line.

tests/test_oom_cpu.py requires TABLE to match the call sites the scanner of tests/poison_sites.py finds (the scanner is imported, not
copied), so a site that is added, moved or removed without its row fails there; tests/test_gpu_oom.py refuses every request of every
statement in turn on the device.  A site that TOLERATES a refusal by design (its caller sees NX_OK and the same words, e.g. after falling
back to a smaller batch) carries the reason in `tolerates`; the sweep accepts NX_OK only from the entries listed in TOLERATING_ENTRIES."""
import collections

from poison_sites import CSRC, ROOT, scan_sites  # noqa: F401  (the scanner, unchanged)

# Site(file, function, calls, owner, caller_sees, tolerates)
#   owner:       what holds the blocks taken earlier in the function while the refused request unwinds — an RAII wrapper by its type, or
#                the named free on the error path; "none earlier" where the function takes one block
#   caller_sees: the return of the function and the state it leaves
#   tolerates:   None, or why the caller still sees NX_OK and equal words
Site = collections.namedtuple("Site", "file function calls owner caller_sees tolerates")
TABLE = []


def site(file, function, calls, owner, caller_sees, tolerates=None):
    TABLE.append(Site(file, function, calls, owner, caller_sees, tolerates))


_ONE = "none earlier: the function takes one block"
_RC = "NX_ERR_OOM as its return code, nothing launched with the pointer that was not handed out"

# ---- the wrappers
site("ctx.hip", "nx_alloc", 1, _ONE, "NX_ERR_OOM, *d_out NULL")
site("prover.h", "alloc", 1, "DevBuf: release() of the block it held before, then its destructor wherever the owner unwinds", "DevBuf::alloc returns the code, p is NULL")
site("prover.h", "alloc_rows", 1, "SecureColumn::buf (a DevBuf)", "the code through H_TRY before fix(): no coordinate pointer is derived from a NULL base that a kernel is given")
site("merkle.hip", "alloc", 1, "RootPipe::bufs: ~RootPipe drains the hash stream and ctx->stream, then dev_free of each in the order they were taken", "RootPipe::alloc returns the code")

# ---- ctx.hip
site("ctx.hip", "nx_gather", 1, _ONE, _RC + "; h_out untouched")

# ---- fft.hip
site("fft.hip", "nx_twiddles_create", 4, "dev_free of d_tw, d_itw, d_tw2, d_itw2 (NULL ones skipped), delete of the handle", "NX_ERR_OOM, *out NULL, twiddle_kernel not launched")
site("fft.hip", "twiddles_first_part", 4, "dev_free of the four tables, delete of the handle", "the code; *out untouched (the callers start from a NULL handle in a guard)")
site("fft.hip", "HostFeed::begin", 1, "HostFeed::finish (its destructor, TreeBuilder's destructor): both feed queues drained, then dev_free of d_tmp[0..1]",
     "the code; no copy queued; upload_columns / TreeBuilder::commit_begin return it")
site("fft.hip", "HostFeed::chunk", 1, "HostFeed::finish, as in begin: the copies of the chunk's earlier columns are drained before d_tmp goes back",
     "the code before the column's copy is queued; the destination columns hold what had arrived")

# ---- merkle.hip
site("merkle.hip", "tree_alloc", 1, "none earlier; delete of the nx_tree", "the code, *out untouched (TreeRef / FriLayer start from NULL)")
site("merkle.hip", "tree_pipe_begin", 1, "none earlier; delete of the nx_tree", "the code, tp->tree stays NULL: PipeGuard of commit_begin has nothing to destroy")
site("merkle.hip", "nx_merkle_commit", 1, "none earlier; delete of the nx_tree", "NX_ERR_OOM, *out NULL, no layer kernel launched")
site("merkle.hip", "nx_commit_root", 4, "RootPipe (see alloc): extension buffers, state, scratch and ring slots taken so far", "NX_ERR_OOM, root untouched; the columns may already hold coefficients (documented: consumed)")
site("merkle.hip", "nx_merkle_from_leaves", 1, "none earlier; delete of the nx_tree", "NX_ERR_OOM, *out NULL")
site("merkle.hip", "nx_grind", 1, _ONE, _RC + "; *nonce untouched")

# ---- pcs.hip
site("pcs.hip", "eval_at_points_enqueue", 1, "the EvalJob list of the caller: eval_at_points_collect drains ctx->stream and gives every queued job's blob and pinned block back — "
     "nx_eval_at_points always collects, prove_core collects on the refusal before it returns", "the code; the jobs queued before it are complete and freed")
site("pcs.hip", "accumulate_quotients_coeffs", 2, "dev_free(comb) on the refusal of ext", "the code, neither kernel launched")

# ---- backend_ops.hip, constraints.hip
site("backend_ops.hip", "nx_fri_decompose", 1, _ONE, _RC + "; lambda and d_g4 untouched")
site("constraints.hip", "nx_eval_constraint_program", 1, _ONE, _RC + "; the accumulator untouched")

# ---- logup.hip, air_jit.hip
site("logup.hip", "logup_cols_launch", 1, _ONE, "the code; nx_logup_cols* return it, the output columns untouched")
site("logup.hip", "nx_logup_finalize_last_batch", 1, _ONE, _RC + "; claimed_sums untouched, the columns not yet scanned")
site("air_jit.hip", "nx_logup_program", 1, _ONE, _RC + "; the output columns untouched")
site("air_jit.hip", "air_check_component", 1, _ONE, "the code; nx_air_check / nx_prover_check return it, no report written")

# ---- the counting entries
site("multiplicity.hip", "nx_logup_multiplicities", 1, _ONE, _RC + "; d_out untouched")
site("multiplicity_sparse.hip", "nx_logup_multiplicities_sparse", 1, _ONE, _RC + "; d_out untouched")
site("access_history.cuh", "access_history", 1, _ONE, "the code; nx_trace_prev_access / nx_trace_access_chain return it, no output column written")
site("trace_partition.hip", "nx_trace_partition_create", 2, "dev_free(p->d_order) on the refusal of the control blob; the unique_ptr deletes the handle", "NX_ERR_OOM, *out NULL, counts untouched")

# ---- comm_local.hip
site("comm_local.hip", "cb_allreduce_m31", 2, "the Free guard: nx_free of snap and pulled", "the callback fails and breaks the group (fail): every rank's collective returns an error, nobody waits")

# ---- machine.hip
site("machine.hip", "fill_and_extend", 1, "DevBuf slab; the TreeBuilder owns the groups queued before", "the code; prove_synth returns it, the trees committed so far die with the CommitmentSchemeProver")
site("machine.hip", "prove_machine", 8, "DevBuf everywhere (kept[], slab, rows, last, recv); TwGuard the twiddles; TreeBuilder tb0 / tb1 / tb2 their groups and host feeds — their "
     "destructors drain the feed queues before the slabs go back; the CommitmentSchemeProver the committed trees",
     "NX_ERR_OOM from nx_prove_machine*, *proof_words untouched (NULL in the caller); row-sharded: abort_peers tells the transport also before the first collective")

# ---- prover.hip
site("prover.hip", "Dist::allgather_cols", 2, "DevBuf send, tmp", "the code before the collective is entered: the entry point aborts the transport")
site("prover.hip", "upload_owned", 1, "the caller's DevBuf", "the code, nothing staged")
site("prover.hip", "TreeBuilder::commit_begin", 1, "the local CommitmentTreeProver (slabs and extensions of the runs done), DevBuf lde, PipeGuard (drains ctx->stream, destroys the begun "
     "nx_tree), TreeBuilder::feeds (finish() in its destructor)", "the code; no tree is appended to the scheme, the channel is untouched")
site("prover.hip", "TreeBuilder::commit_dist", 4, "DevBuf lde, rows, the chunks' send buffers; the local CommitmentTreeProver", "the code; the session / prove entry aborts the transport")
site("prover.hip", "gather_secure", 1, "SecureColumn whole (the caller's)", "the code before the all-gather")
site("prover.hip", "commit", 5, "DevBuf d_state, SecureColumn layer / next / fin, the FriLayer vector tl (TreeRef destroys a tree it holds), FriProver::inner", "the code; prove_core returns it, the channel of a "
     "session is restored by nx_prover_prove")
site("prover.hip", "commit_host_channel", 4, "SecureColumn layer / next, FriProver::inner", "the code; prove_core returns it, as from commit")
site("prover.hip", "sharded_evaluate_exchange", 3, "DevBuf rows, ext, send", "the code before the exchange is entered; the prove entry aborts the transport")
site("prover.hip", "columns_on_eval_domain", 2, "DevBuf ext, whole; EvalDomainCols::keep", "the code; compute_composition returns it before any constraint kernel of the component is launched")
site("prover.hip", "composition_accumulator", 2, "the map of SecureColumn accumulators of the caller", "the code; *out untouched, no kernel adds into an accumulator that was not handed out")
site("prover.hip", "finalize_accumulation", 1, "DevBuf lifted; the accumulator map", "the code; out_polys untouched")
site("prover.hip", "prove_core", 2, "SecureColumn qc and the vector of quotient columns; FriProver; the composition tree already appended is popped by nx_prover_prove / dies with prove_machine's scheme",
     "the code; words untouched")
site("prover.hip", "half_group_finish", 1, "the caller's SecureColumn out_coef; HalfGroup's accumulators", "the code; the half-domain part is not added to the coefficients")
site("prover.hip", "quarter_group_finish", 4, "DevBuf fq, f0q, g; the caller's out_coef", "the code; the quarter-domain part is not added to the coefficients")
site("prover.hip", "GenericAir::compute_composition", 12, "SecureColumn / DevBuf members of the half and quarter groups, DevBuf ext / extm / wholem / wv, SecureColumn full, the accumulator maps",
     "the code; prove_core returns it before the composition tree is committed")
site("prover.hip", "nx_prover_tree_begin", 1, "nx_prover::pending is cleared: the DevBuf slabs of the runs taken so far go back", "NX_ERR_OOM, every d_cols_out entry NULL, the tree not begun: begin again")
site("prover.hip", "nx_prover_check", 1, "DevBuf scratch of the component at hand (the earlier components' were released)", "NX_ERR_OOM, no report written, the session untouched")

# public entries whose refused request is tolerated somewhere below them: {entry: reason}.  None was found: every site above hands the code up.
TOLERATING_ENTRIES = {}
