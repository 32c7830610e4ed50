"""The audit behind the context option "debug.poison": every place under csrc/ that takes a block from the caching allocator
(dev_alloc, nx_alloc, DevBuf::alloc and the wrappers built on it), the regions of the block, and what writes each region IN FULL before
its first reader — a staged upload, a memset, or a named kernel whose every block or lane stores it.  A region nobody reads before its
first writer may hold anything; with the option on it holds the pattern.  Rows cite functions and kernels by name, never by line.

tests/test_poison_cpu.py counts the call sites per enclosing function in the sources (scan_sites) and requires TABLE to match, so an
allocation site that is added, moved or removed without its row fails there; tests/test_gpu_poison.py runs the entries on poisoned
blocks against the oracle.  SWEEP lists the public entries that sweep covers."""
import collections
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nexus-zkvm_amd", "csrc")

# a call that takes a block: the allocator itself, the C entry on top of it, and the owning wrappers' methods (DevBuf::alloc,
# SecureColumn::alloc / alloc_rows, the root plan's alloc of merkle.hip)
ALLOC_CALL = re.compile(r"(?<!int )\b(?:dev_alloc|nx_alloc)\(|(?:\.|->)alloc(?:_rows)?\(")
_NOT_A_NAME = {"if", "for", "while", "switch", "return", "else", "do", "case", "catch", "sizeof", "defined"}
# a function definition that starts a line at indentation 0 (free functions, out-of-class methods) or 4 (methods in a struct body):
# anything but ; { } # up to the name, the parameter list (may span lines), then the opening brace
_DEFINITION = re.compile(r"^(?: {4})?(?![ }#/])[^\n;{}#]*?\b([A-Za-z_~][\w:]*)\s*\(([^;{}]*)\)\s*(?:const\s*)?(?:noexcept\s*)?(?:override\s*)?\{", re.M)


def _blank(match):
    return " " * len(match.group(0))


def scan_file(path):
    """[(enclosing function, line number)] of every allocation call of one source file"""
    text = open(path).read()
    text = re.sub(r"//[^\n]*", _blank, text)
    text = re.sub(r"__launch_bounds__\(\w+\)", _blank, text)
    defs = [(m.start(), m.group(1)) for m in _DEFINITION.finditer(text)
            if m.group(1) not in _NOT_A_NAME and "](" not in m.group(2)]          # ](: a call that ends in a lambda's body, not a definition
    out = []
    for m in ALLOC_CALL.finditer(text):
        owner = [name for pos, name in defs if pos <= m.start()]
        out.append((owner[-1] if owner else None, text.count("\n", 0, m.start()) + 1))
    return out


def scan_sites():
    """{(file, function): number of allocation calls} over csrc/*.hip, *.h, *.cuh"""
    counts = collections.Counter()
    for ext in ("hip", "h", "cuh"):
        for path in sorted(glob.glob(os.path.join(CSRC, "*." + ext))):
            for fn, _ in scan_file(path):
                counts[(os.path.basename(path), fn)] += 1
    return dict(counts)


# ------------------------------------------------------------------------------------------------------------------ the table
# Site(file, function, calls, regions): `calls` allocation calls in `function` of `file`; regions: (what part of the block(s), who
# writes all of it before its first reader).  "never read": no kernel or copy reads those words before the block is freed.
Site = collections.namedtuple("Site", "file function calls regions")
TABLE = []


def site(file, function, calls, *regions):
    TABLE.append(Site(file, function, calls, tuple(regions)))


_PAD = ("the rounding of each part and of the block", "never read")

# ---- the wrappers: they forward, the rows of their callers say who writes the block
site("ctx.hip", "nx_alloc", 1, ("the caller's block", "the caller (the C entry: a test, a binding, DevBuf::alloc)"))
site("prover.h", "alloc", 1, ("DevBuf::alloc: the owner's block", "the owner: the rows of machine.hip / prover.hip below"))
site("prover.h", "alloc_rows", 1, ("SecureColumn::alloc / alloc_rows: 4 coordinate columns of `rows` words", "the owner: the rows of prover.hip below"))
site("merkle.hip", "alloc", 1, ("RootPipe::alloc: one buffer of nx_commit_root", "see nx_commit_root"))

# ---- ctx.hip
site("ctx.hip", "nx_gather", 1,
     ("n pointers, n indices", "upload_async_staged of d_ptrs and of index (n * 8 bytes each)"),
     ("n output words", "gather_kernel: lane i < n stores out[i]; copy_d2h_blocking reads n words"), _PAD)

# ---- fft.hip
site("fft.hip", "nx_twiddles_create", 4, ("d_tw, d_itw, d_tw2, d_itw2: 2^log_half words each", "twiddle_kernel: every lane stores its 4 words of all four tables, the pad word included"))
site("fft.hip", "twiddles_first_part", 4, ("d_tw, d_itw, d_tw2, d_itw2: 2^(n-1) words each", "sub_twiddle_kernel: lane i < 2^(n-1) stores word i of all four tables (the last lane the pad word)"))
site("fft.hip", "HostFeed::begin", 1,
     ("d_tmp[0..1], coset order: 2^log words each", "HostFeed::chunk: hipMemcpyAsync of the whole column on copy_stream, behind the event begin() records on ctx->stream after the "
      "allocation; finalize_kernel reads it behind copied[k]"))
site("fft.hip", "HostFeed::chunk", 1,
     ("d_tmp[k], first narrow column of a circle-order feed: 2^log words", "hipMemcpyAsync of the column's 2^log * W bytes on the slot's queue, behind the event recorded on ctx->stream "
      "after the allocation; widen_kernel reads those bytes only"))

# ---- merkle.hip
site("merkle.hip", "tree_alloc", 1,
     ("layers max_log .. 0 of a fused commit (merkle_commit_fused, fri_fold_commit_fused) or of a FRI tail tree", "merkle_fused_kernel stores the leaf layer and 6 levels, "
      "merkle_subtree_kernel / merkle_layer_kernel / merkle_top_kernel the levels above; fri_tail_kernel stores every layer of its trees"))
site("merkle.hip", "tree_pipe_begin", 1,
     ("leaf layer", "leaf_chain_launch (tree_pipe_absorb): the first block of columns takes no state in, every later one reads the state the one before stored"),
     ("inner layers", "build_inner_layers: merkle_layer_kernel / merkle_subtree_kernel / merkle_top_kernel store every node of a layer from the layer below"))
site("merkle.hip", "nx_merkle_commit", 1,
     ("leaf layer", "merkle_layer_kernel (prev = NULL): lane i < 2^max_log stores node i"),
     ("inner layers", "build_inner_layers, as in tree_pipe_begin"))
site("merkle.hip", "nx_commit_root", 4,
     ("extension of the smaller columns, one buffer per size", "nx_lde_batch stores every extended column whole"),
     ("state: 2^el nodes", "leaf_chain_launch on the hash stream, behind ev_lde[s], which is recorded on ctx->stream after the allocations; chunk 0 takes no state in"),
     ("scratch: root_scratch_nodes nodes", "reduce_to_root: every launch stores all nodes of the level it produces and the next reads only those"),
     ("ring[s]: 16 extended columns", "nx_lde_batch of the chunk; the leaf chain reads it behind ev_lde[s]"),
     ("the release", "~RootPipe drains the hash stream and ctx->stream before dev_free"))
site("merkle.hip", "nx_merkle_from_leaves", 1,
     ("leaf layer", "nx_copy of the caller's 2^log digests"),
     ("inner layers", "merkle_layer_kernel per level down to merkle.top, merkle_top_kernel the rest"))
site("merkle.hip", "nx_grind", 1, ("digest (8 words) and result (u64 = ~0)", "hipMemcpyAsync of the whole 40-byte struct"), _PAD)

# ---- pcs.hip
site("pcs.hip", "eval_at_points_enqueue", 1,
     ("d_lo, d_hi: the two factor tables", "eval_tables_kernel: lane i < n_lo + n_hi stores its 4 words"),
     ("d_part: np * n_chunks * 4 partial sums", "eval_at_point_kernel: block (chunk, poly) stores its 4 words; the copy to h_part reads exactly those"))
site("pcs.hip", "accumulate_quotients_coeffs", 2,
     ("comb: n_slices slices of 4 n_batches combined coefficient columns", "quotient_combine_kernel: block (x, slice) stores every combination of its rows; quotient_combine_reduce_kernel adds the slices into slice 0"),
     ("ext: 4 n_batches extended columns", "nx_evaluate_batch stores every output column whole; quotient_finish_kernel reads them"))

# ---- backend_ops.hip, constraints.hip
site("backend_ops.hip", "nx_fri_decompose", 1,
     ("n_blocks * 4 partial sums", "decompose_sum_kernel: lanes 0..3 of every block store the block's 4 words"),
     ("lambda: 4 words", "decompose_lambda_kernel: lanes 0..3"))
site("constraints.hip", "nx_eval_constraint_program", 1,
     ("program, column table, secure constants, alpha powers, denominators", "upload_async_staged of each (an empty part is skipped and never read: the validated program cannot index it)"), _PAD)

# ---- logup.hip, air_jit.hip
site("logup.hip", "logup_cols_launch", 1, ("fraction descriptors, tuple column table, alpha powers, output table", "stage + hipMemcpyAsync of the whole zero-initialised host image (`total` bytes)"), _PAD)
site("logup.hip", "nx_logup_finalize_last_batch", 1,
     ("d_tab: n_cols Sec4", "hipMemcpyAsync of the host table"),
     ("d_sums: n_cols * n_blocks * 4", "logup_scan_local_kernel: the last lane of block (b, col) stores its 4 totals; tiled: logup_scan_tile_kernel, lane j == 7 of every segment of every "
      "(column, coordinate) stores its total — the segments of the tiles cover 0 .. n_blocks - 1"),
     ("d_meta: 8 words per column", "logup_scan_sums_kernel: the last lane of the column's block stores all 8"))
site("air_jit.hip", "nx_logup_program", 1, ("column table, secure constants, output table", "stage + hipMemcpyAsync of the whole zero-initialised host image"), _PAD)
site("air_jit.hip", "air_check_component", 1,
     ("column table, secure constants, count[] = 0, first[] = ~0", "upload_async_staged of the whole host image: the counters and the atomicMin slots start from it"), _PAD)

# ---- the counting entries (their host twins run on blocks filled with 0xA5A5A5A5: tests/native/*_emul)
site("multiplicity.hip", "nx_logup_multiplicities", 1,
     ("MultCtl (first_missing, tab_oor_pos, tab_dup_key = ~0), uses, tile starts", "upload_async_staged of each"),
     ("d_cnt: 2^total_bits u64 counters", "hipMemsetAsync before mult_count_kernel"), _PAD)
site("multiplicity_sparse.hip", "nx_logup_multiplicities_sparse", 1,
     ("MsCtl (first_missing, tab_dup, tab_oor_pos = ~0), uses, tile starts", "upload_async_staged of each"),
     ("d_k / d_v pairs", "count_pass: pass 0 reads the table and scatters into pair 0 (count_place_kernel: every element), each later pass into the other pair"),
     ("d_hist", "count_hist_kernel: each block writes its whole histogram"),
     ("d_cnt (the pair the last pass has read)", "hipMemsetAsync before ms_count_kernel"),
     ("d_split", "ms_split_kernel: every lane < MS_LDS_KEYS stores its splitter (tables the LDS holds whole use d_k instead)"), _PAD)
site("access_history.cuh", "access_history", 1,
     ("AhCtl (first_bad = ~0), streams, epochs, tile starts, bases, payload / prev tables, rules, deltas", "upload_async_staged of each"),
     ("d_k[0] / d_v[0]", "ah_enumerate_kernel: every lane of every tile stores its element (AH_NONE for a row that does not access)"),
     ("d_k[1] / d_v[1]", "count_pass: count_place_kernel scatters every element of the pass"),
     ("d_hist", "count_hist_kernel: each block writes its whole histogram"),
     ("d_cnt, d_last, d_aset, d_aval: one word per resolve block (and chain op)", "ah_heads_kernel: every block stores its words; scan_kernel / ah_scan_ops_kernel scan them in place"), _PAD)
site("trace_partition.hip", "nx_trace_partition_create", 2,
     ("d_order: n_steps words", "count_pass with TpOrder: count_place_kernel stores the place of every step"),
     ("TpCtl (first_bad = ~0)", "upload_async_staged; start[] and total by count_pass's scan"),
     ("d_hist", "count_hist_kernel: each block writes its whole histogram"), _PAD)

# ---- comm_local.hip
site("comm_local.hip", "cb_allreduce_m31", 2,
     ("snap", "nx_copy of the rank's buffer, then nx_sync, before any peer may pull it"),
     ("pulled", "hipMemcpyAsync of a peer's snapshot on the transport's stream, after that nx_sync; nx_m31_add_into reads it after the stream's synchronisation"))

# ---- machine.hip
site("machine.hip", "fill_and_extend", 1, ("the component's columns of one synthetic tree", "synth_fill_range: synth_fill_kernel stores every row of every column"))
site("machine.hip", "prove_machine", 8,
     ("kept buffers (one GPU / row-sharded)", "synth_fill_range into the kept column, or HostFeed::chunk (keep list); the commit's inverse transform reads them"),
     ("trace slab, device fill", "synth_fill_range for the columns that are not kept; a kept column's place is first written by the commit's transform (lde_batch_from: coefficients to `cols`)"),
     ("trace slab, host columns", "HostFeed::chunk uploads every column behind the event HostFeed::begin records after the allocation"),
     ("rows: every logup column", "logup_columns: logup_cols_kernel / the logup program's kernels store every row of every coordinate column"),
     ("last, recv, slab (row-sharded)", "Dist::allgather_cols, Dist::alltoallv, transpose_blocks (unpack) and nx_copy store them whole"))

# ---- prover.hip
site("prover.hip", "Dist::allgather_cols", 2, ("send", "nx_copy of every block"), ("tmp", "allgather_dev stores world * n * rb words; transpose_blocks reads them"))
site("prover.hip", "upload_owned", 1, ("n_words words", "stage + hipMemcpyAsync in chunks"), ("up to 4 words of padding", "never read"))
site("prover.hip", "TreeBuilder::commit_begin", 1, ("lde: the run's extended columns", "lde_batch_from / nx_evaluate_batch store every output column whole; the leaf chain and the inner layers read them behind it"))
site("prover.hip", "TreeBuilder::commit_dist", 4,
     ("lde (replicated polynomials / a chunk's share)", "nx_evaluate_batch / nx_lde_batch"),
     ("send of a chunk", "transpose_blocks (pack) stores all of it; the exchange waits for the event recorded behind it"),
     ("rows", "Dist::alltoallv stores every received block"))
site("prover.hip", "gather_secure", 1, ("the whole secure column", "Dist::allgather_cols: transpose_blocks (unpack) stores every row of the 4 coordinates"))
site("prover.hip", "commit", 5,
     ("d_state: head of 9 words", "stage + nx_copy of digest and n_sent = 0"),
     ("d_state: record j", "fri_channel_kernel stores root and alpha of record j before the fold that reads rec_alpha(j); fri_tail_kernel stores the records of its layers; only the "
      "records written are downloaded"),
     ("layer (the first line layer)", "nx_memset_zero: the circle columns fold INTO it"),
     ("tail evaluations, fin", "fri_tail_kernel stores every layer it folds"),
     ("next", "fold_line_dev or fri_fold_commit_fused stores every point before the layer's commit reads it"))
site("prover.hip", "commit_host_channel", 4,
     ("layer", "nx_memset_zero"), ("next", "fold_line_rows / nx_fold_line store every point (of the block)"))
site("prover.hip", "sharded_evaluate_exchange", 3,
     ("ext", "nx_evaluate_batch"), ("send", "transpose_blocks (pack)"), ("rows", "Dist::alltoallv stores every block that is handed out in *blk"))
site("prover.hip", "columns_on_eval_domain", 2,
     ("ext: the re-evaluated columns", "nx_evaluate_batch stores ns columns whole (ns == 0: one word, never read)"), ("whole: the neighbour-read columns", "Dist::allgather_cols"))
site("prover.hip", "composition_accumulator", 2, ("the accumulator of one size", "nx_memset_zero: the constraint kernels add into it"))
site("prover.hip", "finalize_accumulation", 1, ("lifted: the running polynomial on the next size", "nx_evaluate_batch stores the 4 columns whole"))
site("prover.hip", "prove_core", 2, ("qc: the quotient of one size group", "quotient_kernel / quotient_small_kernel store every row of the 4 coordinates (of the block); via coefficients: quotient_finish_kernel"))
site("prover.hip", "half_group_finish", 1, ("out_coef: 2N coefficients per coordinate", "nx_memset_zero, then nx_copy / the fix-up kernel"))
site("prover.hip", "quarter_group_finish", 4,
     ("fq, g", "axpy_scale stores N words per coordinate"), ("f0q", "nx_evaluate_batch"), ("out_coef", "nx_memset_zero, then nx_copy and half_fix_kernel"))
site("prover.hip", "GenericAir::compute_composition", 12,
     ("hg.acc, qg.acc2n, qg.accq, qg.rown, full: accumulators", "nx_memset_zero right behind each allocation: air_eval_rows adds into them"),
     ("ext, extm, wholem: re-evaluated columns", "nx_evaluate_batch / Dist::allgather_cols store every column the kernel is given a pointer to (ns == 0: one word, never read)"),
     ("wv: the columns' values at row N", "nx_upload of ns words; only those are pointed at"))
site("prover.hip", "nx_prover_tree_begin", 1, ("the slab of one run of equally sized columns", "the caller, through the pointers the entry returns (a trace fill, nx_upload, nx_logup_cols), before nx_prover_tree_commit"))
site("prover.hip", "nx_prover_check", 1, ("scratch: evaluations of the columns that were committed as polynomials", "nx_evaluate_batch stores each whole before the checker's kernels read it"))


# ------------------------------------------------------------------------------------------------------------------ the sweep
# The public entries tests/test_gpu_poison.py runs on poisoned blocks: every entry of placement.TABLE, and these.
SWEEP_EXTRA = (
    "nx_alloc", "nx_free", "nx_ctx_memory",
    "nx_logup_multiplicities_sparse", "nx_trace_access_chain", "nx_trace_partition_create", "nx_gather", "nx_grind",
    "nx_merkle_decommit", "nx_merkle_layer", "nx_merkle_root", "nx_air_check", "nx_prover_check", "nx_synth_fill_tree", "nx_generate_secure_powers",
    "nx_prove_synth", "nx_prove_machine", "nx_prove_machine_host", "nx_prove_machine_host_narrow", "nx_prover_create", "nx_prover_tree_begin", "nx_prover_tree_commit",
    "nx_prover_tree_commit_host", "nx_prover_tree_share", "nx_prover_tree_adopt", "nx_prover_prove", "nx_comm_local_create",
)
