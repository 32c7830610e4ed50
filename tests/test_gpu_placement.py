"""Every device entry at column placements the allocator never makes (tests/placement.py holds the arena, the classification table, the
case list and the oracle side).  A case's columns lie in ONE slab from nx_alloc at chosen word offsets modulo 4 between guards of
0xDEADBEEF; after the call the slab is downloaded and judged: guards intact, inputs byte-identical, outputs bit-equal to the oracle.

S and B entries run at every shift.  W entries run where include/nexus_hip.h allows (their short, word-kernel sizes at every shift; their
word-access arguments shifted; 8-byte arguments at 0 and 2 words); at a forbidden offset the test asserts the refusal — NX_ERR_ARG naming
the argument and the column, no word of the slab changed, and the same call, aligned, correct on the same context afterwards.  No kernel
is ever launched on a pointer the header forbids."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import oracle_lib as O
import placement as PL

pytestmark = pytest.mark.gpu
NX_ERR_ARG = -2


@pytest.fixture(scope="module")
def nz():
    import nexus_zkvm_amd
    return nexus_zkvm_amd


@pytest.fixture(scope="module")
def be(nz):
    b = nz.HipBackend(0)
    b.tw = b.precompute_twiddles(PL.TW_LOG)
    b.kernels = {}
    yield b
    for k in b.kernels.values():
        k.close()
    b.tw = None
    b.close()


def PA(addrs):
    return (C.c_void_p * max(1, len(addrs)))(*[int(a) if a else None for a in addrs])


def u32p(a):
    return a.ctypes.data_as(C.c_void_p)


class Ptrs:
    """a list of column pointers where a binding method wants something with col_ptrs()"""

    def __init__(self, addrs):
        self.addrs = list(addrs)

    def col_ptrs(self):
        return PA(self.addrs)


class Slab:
    """the arena of a plan on the device"""

    def __init__(self, be, plan):
        self.be, self.arena = be, plan.arena
        self.ptr = C.c_void_p()
        be._chk(be.L.nx_alloc(be.ctx, C.c_size_t(self.arena.size), C.byref(self.ptr)))
        assert self.ptr.value % 256 == 0
        img = self.arena.image()
        be._chk(be.L.nx_upload(be.ctx, self.ptr, u32p(img), C.c_size_t(img.size)))

    def __call__(self, name, word=0):
        return self.ptr.value + 4 * self.arena.offset(name, word)

    def cols(self, prefix, n):
        return [self(f"{prefix}{k}") for k in range(n)]

    def coords(self, name, log):
        """the 4 coordinate columns packed in one slab column"""
        return [self(name, q << log) for q in range(4)]

    def download(self):
        self.be.sync()
        out = np.empty(self.arena.size, np.uint32)
        self.be._chk(self.be.L.nx_download(self.be.ctx, u32p(out), self.ptr, C.c_size_t(out.size)))
        return out

    def free(self):
        self.be.L.nx_free(self.be.ctx, self.ptr)


def tree_words(be, nz, h, max_log):
    t = nz.MerkleTree(be, h)
    root = t.root()
    layers = np.concatenate([t.layer(k).reshape(-1) for k in range(max_log, -1, -1)])
    return {"root": root, "layers": layers}


# ---------------------------------------------------------------------------------------------------------------- the runners
RUN = {}


def runs(name):
    def deco(fn):
        RUN[name] = fn
        return fn
    return deco


@runs("nx_interpolate_batch")
def _(be, nz, p, A):
    a = p.args
    be._chk(be.L.nx_interpolate_batch(be.ctx, be.tw.h, PA(A.cols("col", a["n_cols"])), a["n_cols"], a["log"]))


@runs("nx_evaluate_batch")
def _(be, nz, p, A):
    a = p.args
    be._chk(be.L.nx_evaluate_batch(be.ctx, be.tw.h, PA(A.cols("poly", a["n_cols"])), a["n_cols"], a["log"], a["log_expand"], PA(A.cols("out", a["n_cols"]))))


@runs("nx_lde_batch")
def _(be, nz, p, A):
    a = p.args
    be._chk(be.L.nx_lde_batch(be.ctx, be.tw.h, PA(A.cols("col", a["n_cols"])), a["n_cols"], a["log"], a["log_blowup"], PA(A.cols("lde", a["n_cols"]))))


@runs("nx_lde_commit")
def _(be, nz, p, A):
    a, root = p.args, np.zeros(8, np.uint32)
    be._chk(be.L.nx_lde_commit(be.ctx, be.tw.h, PA(A.cols("col", a["n_cols"])), a["n_cols"], a["log"], a["log_blowup"], PA(A.cols("lde", a["n_cols"])), u32p(root)))
    return {"root": root}


@runs("nx_commit_root")
def _(be, nz, p, A):
    a, root = p.args, np.zeros(8, np.uint32)
    logs = np.array(a["logs"], np.uint32)
    be._chk(be.L.nx_commit_root(be.ctx, be.tw.h, PA(A.cols("col", len(logs))), u32p(logs), len(logs), a["log_blowup"], u32p(root)))
    return {"root": root}


@runs("nx_merkle_commit")
def _(be, nz, p, A):
    a = p.args
    logs, h = np.array(a["logs"], np.uint32), C.c_void_p()
    fused0 = be.get_option("merkle.fused")
    be.set_hash_mode(a["mode"])
    be.set_option("merkle.fused", PL.FUSED_LOG)          # the fused launch from 2^12 rows (default: 2^21), so that its host branch is reached at a test size
    try:
        be._chk(be.L.nx_merkle_commit(be.ctx, PA(A.cols("col", len(logs))), u32p(logs), len(logs), C.byref(h)))
        return tree_words(be, nz, h, int(logs.max()))
    finally:
        be.set_hash_mode(0)
        be.set_option("merkle.fused", fused0)


@runs("nx_merkle_commit_on_layer")
def _(be, nz, p, A):
    a = p.args
    be.set_hash_mode(a["mode"])
    try:
        be._chk(be.L.nx_merkle_commit_on_layer(be.ctx, a["log"], C.c_void_p(A("prev")) if a["has_prev"] else None, PA(A.cols("col", a["n_cols"])) if a["n_cols"] else None,
                                               a["n_cols"], C.c_void_p(A("out"))))
    finally:
        be.set_hash_mode(0)


@runs("nx_merkle_leaf_chain")
def _(be, nz, p, A):
    a = p.args
    cols, state = A.cols("col", 20), C.c_void_p(A("state"))
    be.set_hash_mode(a["mode"])
    try:
        if not (p.case.refuse and p.case.refuse[0] == "d_state_in"):      # (a misaligned d_state_in can only be passed by a shard behind the first)
            be._chk(be.L.nx_merkle_leaf_chain(be.ctx, PA(cols[:16]), 16, a["log"], 0, 20, None, state, C.c_uint64(0), C.c_uint64(1 << a["log"])))
        be._chk(be.L.nx_merkle_leaf_chain(be.ctx, PA(cols[16:]), 4, a["log"], 16, 20, state, state, C.c_uint64(0), C.c_uint64(1 << a["log"])))
    finally:
        be.set_hash_mode(0)


@runs("nx_merkle_from_leaves")
def _(be, nz, p, A):
    a, h = p.args, C.c_void_p()
    be.set_hash_mode(a["mode"])
    try:
        be._chk(be.L.nx_merkle_from_leaves(be.ctx, C.c_void_p(A("leaves")), a["log"], C.byref(h)))
        return tree_words(be, nz, h, a["log"])
    finally:
        be.set_hash_mode(0)


@runs("nx_eval_at_points")
def _(be, nz, p, A):
    a = p.args
    idx, pts, out = np.array(a["idx"], np.uint32), np.ascontiguousarray(np.stack(a["points"]), dtype=np.uint32), np.zeros((len(a["idx"]), 4), np.uint32)
    be._chk(be.L.nx_eval_at_points(be.ctx, PA(A.cols("poly", a["n_cols"])), a["log"], u32p(idx), u32p(pts), len(idx), u32p(out)))
    return {"values": out}


def _quotient_args(p, A):
    a = p.args
    keep = [np.ascontiguousarray(a[k], dtype=np.uint32) for k in ("alpha", "points", "counts", "cidx", "values")]
    return keep, (a["log"], PA(A.cols("col", a["n_cols"])), a["n_cols"], u32p(keep[0]), 2, u32p(keep[1]), u32p(keep[2]), u32p(keep[3]), u32p(keep[4]))


@runs("nx_accumulate_quotients")
def _(be, nz, p, A):
    keep, args = _quotient_args(p, A)
    be._chk(be.L.nx_accumulate_quotients(be.ctx, *args, PA(A.cols("out", 4))))


@runs("nx_accumulate_quotients_partial")
def _(be, nz, p, A):
    keep, args = _quotient_args(p, A)
    be._chk(be.L.nx_accumulate_quotients_partial(be.ctx, *args, None, 1, PA(A.cols("out", 4))))


@runs("nx_fold_circle_into_line")
def _(be, nz, p, A):
    log, alpha = p.args["log"], np.ascontiguousarray(p.args["alpha"], dtype=np.uint32)
    be._chk(be.L.nx_fold_circle_into_line(be.ctx, be.tw.h, PA(A.coords("dst", log - 1)), PA(A.coords("src", log)), log, u32p(alpha)))


@runs("nx_fold_line")
def _(be, nz, p, A):
    log, alpha = p.args["log"], np.ascontiguousarray(p.args["alpha"], dtype=np.uint32)
    be._chk(be.L.nx_fold_line(be.ctx, be.tw.h, PA(A.coords("src", log)), log, 0, u32p(alpha), PA(A.coords("dst", log - 1))))


@runs("nx_fri_decompose")
def _(be, nz, p, A):
    log, lam = p.args["log"], np.zeros(4, np.uint32)
    be._chk(be.L.nx_fri_decompose(be.ctx, PA(A.coords("src", log)), log, PA(A.coords("g", log)), u32p(lam)))
    return {"lambda": lam}


@runs("nx_secure_accumulate")
def _(be, nz, p, A):
    log = p.args["log"]
    # the slabs are DeviceColumns views: the binding's own method takes them unchanged
    be.secure_accumulate(nz.DeviceColumns.view(be, A("dst"), 4, log), nz.DeviceColumns.view(be, A("src"), 4, log))


@runs("nx_batch_inverse_m31")
def _(be, nz, p, A):
    a = p.args
    be._chk(be.L.nx_batch_inverse_m31(be.ctx, C.c_void_p(A("src")), C.c_void_p(A("src" if a["alias"] else "dst")), C.c_size_t(a["n"])))


@runs("nx_batch_inverse_qm31")
def _(be, nz, p, A):
    a = p.args
    be._chk(be.L.nx_batch_inverse_qm31(be.ctx, PA(A.coords("src", a["log"])), PA(A.coords("src" if a["alias"] else "dst", a["log"])), C.c_size_t(1 << a["log"])))


@runs("nx_m31_add_into")
def _(be, nz, p, A):
    be._chk(be.L.nx_m31_add_into(be.ctx, C.c_void_p(A("dst")), C.c_void_p(A("src")), C.c_size_t(p.args["n"])))


@runs("nx_m31_widen")
def _(be, nz, p, A):
    be._chk(be.L.nx_m31_widen(be.ctx, C.c_void_p(A("dst")), C.c_void_p(A("src")), C.c_size_t(p.args["n"])))


@runs("nx_m31_narrow")
def _(be, nz, p, A):
    be._chk(be.L.nx_m31_narrow(be.ctx, C.c_void_p(A("dst")), C.c_void_p(A("src")), C.c_size_t(p.args["n"])))


@runs("nx_bit_reverse")
def _(be, nz, p, A):
    be.bit_reverse_column(nz.DeviceColumns.view(be, A("col"), 1, p.args["log"]))


@runs("nx_bit_reverse_secure")
def _(be, nz, p, A):
    be.bit_reverse_secure(nz.DeviceColumns.view(be, A("col4"), 4, p.args["log"]))


@runs("nx_finalize_columns")
def _(be, nz, p, A):
    a = p.args
    be._chk(be.L.nx_finalize_columns(be.ctx, PA(A.cols("src", a["n_cols"])), PA(A.cols("dst", a["n_cols"])), a["n_cols"], a["log"]))


@runs("nx_upload_coset_order")
def _(be, nz, p, A):
    h = np.ascontiguousarray(p.args["host"], dtype=np.uint32)
    be._chk(be.L.nx_upload_coset_order(be.ctx, u32p(h), p.args["log"], C.c_void_p(A("dst"))))


@runs("nx_upload_columns")
def _(be, nz, p, A):
    a = p.args
    arrs = [np.ascontiguousarray(c, dtype=np.uint32) for c in a["host"]]
    be._chk(be.L.nx_upload_columns(be.ctx, *nz._host_columns(arrs, None), len(arrs), a["log"], PA(A.cols("dst", len(arrs))), 1 if a["coset"] else 0))


@runs("nx_upload_columns_narrow")
def _(be, nz, p, A):
    a = p.args
    arrs, kinds = nz._narrow_columns(a["host"])
    be._chk(be.L.nx_upload_columns_narrow(be.ctx, *nz._host_columns(arrs, kinds), len(arrs), a["log"], PA(A.cols("dst", len(arrs))), 1 if a["coset"] else 0))


@runs("nx_copy")
def _(be, nz, p, A):
    be._chk(be.L.nx_copy(be.ctx, C.c_void_p(A("dst")), C.c_void_p(A("src")), C.c_size_t(p.args["n"])))


@runs("nx_logup_combine")
def _(be, nz, p, A):
    a = p.args
    ap, z = np.ascontiguousarray(a["alphas"], dtype=np.uint32).reshape(-1), np.ascontiguousarray(a["z"], dtype=np.uint32)
    be._chk(be.L.nx_logup_combine(be.ctx, PA(A.cols("tuple", a["n_cols"])), a["n_cols"], u32p(ap), u32p(z), a["log"], PA(A.coords("out", a["log"]))))


@runs("nx_logup_finalize_col")
def _(be, nz, p, A):
    log = p.args["log"]
    sa, sb = np.array(PL.MINUS_ONE, np.uint32), np.array((1, 0, 0, 0), np.uint32)
    prev = A.coords("prev", log)
    be._chk(be.L.nx_logup_finalize_col(be.ctx, log, C.c_void_p(A("mult_a")), u32p(sa), PA(A.coords("den_a", log)), C.c_void_p(A("mult_b")), u32p(sb), PA(A.coords("den_b", log)),
                                       PA(prev), PA(prev if p.args["alias"] else A.coords("out", log))))


def _frac_structs(nz, p, A):
    keep, arr = [], (nz.LogupFrac * len(p.args["fracs"]))()
    for i, f in enumerate(p.args["fracs"]):
        ptrs = PA([A(n) for n in f["tuple_names"]])
        ap, z, sc = (np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in (f["alphas"], f["z"], f["scale"]))
        keep += [ptrs, ap, z, sc]
        arr[i] = nz.LogupFrac(C.cast(ptrs, C.c_void_p), len(f["tuple_names"]), u32p(ap), u32p(z), A(f["mult_name"]) if f["mult_name"] else None, u32p(sc))
    return keep, arr


@runs("nx_logup_col")
def _(be, nz, p, A):
    log = p.args["log"]
    keep, arr = _frac_structs(nz, p, A)
    prev = A.coords("prev", log)
    be._chk(be.L.nx_logup_col(be.ctx, log, C.byref(arr[0]), C.byref(arr[1]), PA(prev), PA(prev if p.args["alias"] else A.coords("out", log))))


@runs("nx_logup_cols")
def _(be, nz, p, A):
    log, n = p.args["log"], p.args["n_logup"]
    keep, arr = _frac_structs(nz, p, A)
    be._chk(be.L.nx_logup_cols(be.ctx, log, arr, n, PA([x for j in range(n) for x in A.coords(f"out{j}", log)])))


@runs("nx_logup_cols_batched")
def _(be, nz, p, A):
    log, n = p.args["log"], p.args["n_logup"]
    keep, arr = _frac_structs(nz, p, A)
    b = None if p.args["batching"] is None else np.array(p.args["batching"], np.uint32)
    be._chk(be.L.nx_logup_cols_batched(be.ctx, log, arr, len(p.args["fracs"]), u32p(b) if b is not None else None, n, PA([x for j in range(n) for x in A.coords(f"out{j}", log)])))


@runs("nx_logup_finalize_last")
def _(be, nz, p, A):
    return {"claimed": be.logup_finalize_last(A.coords("col4", p.args["log"]), p.args["log"])}


@runs("nx_logup_finalize_last_batch")
def _(be, nz, p, A):
    log, n = p.args["log"], p.args["n"]
    cs = np.zeros((n, 4), np.uint32)
    be._chk(be.L.nx_logup_finalize_last_batch(be.ctx, log, PA([x for j in range(n) for x in A.coords(f"col4_{j}", log)]), n, u32p(cs)))
    return {"claimed": cs}


@runs("nx_logup_program")
def _(be, nz, p, A):
    a = p.args
    prog = a["program"]
    outs = [A(f"out{j}_{q}") for j in range(prog.n_logup_cols) for q in range(4)]
    be.logup_program(prog, A.cols("col", a["n_in"]) + [None] * (4 * prog.n_logup_cols), a["log"], out_ptrs=outs)


@runs("nx_logup_multiplicities")
def _(be, nz, p, A):
    a = p.args
    uses = [(A.cols("val", 2), A("weight"), a["log"]), (A.cols("second", 2), None, a["log2"])]
    missing = be.logup_multiplicities(uses, A.cols("table", 2), a["log_table"], a["key_bits"], A("mult"))
    assert missing == (0, 0, 0)


@runs("nx_eval_constraint_program")
def _(be, nz, p, A):
    a = p.args
    be.eval_constraint_program(a["program"], A.cols("col", a["n_cols"]), a["pw"], a["den"], a["log"], a["log_eval"], Ptrs(A.cols("acc", 4)))


@runs("nx_air_eval")
def _(be, nz, p, A):
    a = p.args
    if "air" not in be.kernels:
        be.kernels["air"] = be.compile_air(a["program"], a["n_cols"])
    be.kernels["air"].eval(A.cols("col", a["n_cols"]), a["pw"], a["den"], a["log"], a["log_eval"], Ptrs(A.cols("acc", 4)))


@runs("nx_trace_prev_access")
def _(be, nz, p, A):
    a = p.args
    streams = []
    for s in range(a["n_streams"]):
        streams.append(dict(key=A.cols(f"s{s}key", 2), flag=A(f"s{s}flag") if a["has_flag"][s] else None, payload=A.cols(f"s{s}pay", a["n_payload"]),
                            prev=A.cols(f"s{s}prev", a["n_payload"]), ordinal=A(f"s{s}ord"), log_size=a["logs"][s], epoch=0, linear=False))
    return {"n_keys": be.trace_prev_access(streams, a["key_bits"], a["n_payload"], init=a["init"])}


@runs("nx_trace_partition_fill")
def _(be, nz, p, A):
    a = p.args
    counts, part = be.trace_partition(A("class"), a["n_steps"], a["n_classes"])
    try:
        assert np.array_equal(counts, a["counts"])
        part.fill(A.cols("src", 2), [dict(cls=d["cls"], log_size=d["log_size"], cols=A.cols(f"d{i}col", len(d["limbs"])), limbs=d["limbs"], is_pad=A(f"d{i}pad"), step=A(f"d{i}step"))
                                     for i, d in enumerate(a["dests"])])
        be.sync()
    finally:
        part.destroy()


@runs("nx_trace_keccak_round")
def _(be, nz, p, A):
    a = p.args
    be.trace_keccak_round(A("states"), a["n_instances"], a["first_round"], a["log_rounds"], a["log"], A.cols("main", a["n_main"]), A.cols("pre", a["n_pre"]), A("states_out"))


@runs("nx_trace_keccak_memory_check")
def _(be, nz, p, A):
    a = p.args
    be.trace_keccak_memory_check(A("states"), A("addresses"), A("timestamps"), a["n_instances"], a["log"], A.cols("main", a["n_main"]), A.cols("pre", a["n_pre"]), A("states_out"))


@runs("nx_trace_program")
def _(be, nz, p, A):
    a = p.args
    be.trace_program(a["program"], A.cols("col", a["n_cols"]), a["log"])


# ---------------------------------------------------------------------------------------------------------------- the judge

def run_case(be, nz, case):
    plan = PL.build(case)
    A = Slab(be, plan)
    try:
        got = RUN[case.entry](be, nz, plan, A) or {}
        after = A.download()
    finally:
        A.free()
    errs = plan.arena.check(after, plan.expect)
    assert not errs, (PL.case_id(case), errs)
    assert set(got) >= set(plan.host), (PL.case_id(case), sorted(got), sorted(plan.host))
    for k, want in plan.host.items():
        assert np.array_equal(np.asarray(got[k]).reshape(-1), np.asarray(want).reshape(-1)), (PL.case_id(case), k)


def refuse_case(be, nz, case):
    """the W contract: NX_ERR_ARG naming the argument and the column, nothing launched (no word of the slab changed), the context usable"""
    plan = PL.build(case)
    arg, _, index = case.refuse
    A = Slab(be, plan)
    try:
        with pytest.raises(nz.NexusHipError) as e:
            RUN[case.entry](be, nz, plan, A)
        after = A.download()
    finally:
        A.free()
    text = str(e.value)
    assert f"error {NX_ERR_ARG}:" in text, text
    assert (arg if index is None else f"{arg}[{index}]") in text and "aligned" in text, text
    errs = plan.arena.check(after, {})
    assert not errs, (PL.case_id(case), errs)
    run_case(be, nz, case._replace(refuse=None))      # the same call, aligned, on the same context


def check(be, nz, case):
    try:
        if case.refuse:
            refuse_case(be, nz, case)
        else:
            run_case(be, nz, case)
    except nz.NexusHipError as e:
        if "HIP error" in str(e):          # a device error: nothing more is launched on this device by this run
            pytest.exit(f"{PL.case_id(case)}: {e}", returncode=3)
        raise


def _param(family):
    return pytest.mark.parametrize("case", PL.family_cases(family), ids=PL.case_id)


@_param("transforms")
def test_transforms(be, nz, oracle, case):
    check(be, nz, case)


@_param("merkle")
def test_merkle(be, nz, oracle, case):
    check(be, nz, case)


@_param("pcs")
def test_pcs(be, nz, oracle, case):
    check(be, nz, case)


@_param("field")
def test_field_utilities(be, nz, oracle, case):
    check(be, nz, case)


@_param("layout")
def test_copies_and_layout(be, nz, oracle, case):
    check(be, nz, case)


@_param("logup")
def test_logup(be, nz, oracle, case):
    check(be, nz, case)


@_param("air")
def test_air(be, nz, oracle, case):
    check(be, nz, case)


@_param("fills")
def test_fills(be, nz, oracle, case):
    check(be, nz, case)


def test_every_case_has_a_runner():
    assert set(RUN) == set(PL.TABLE)


# ---------------------------------------------------------------------------------------------------------------- the session's slabs

@pytest.mark.parametrize("mode", [0, 1])
def test_session_slab_layout_and_commit_of_packed_small_columns(be, nz, oracle, mode):
    """nx_prover_tree_begin packs a run of equal sizes into one slab: column k of a run sits at base + (k << log), so every second column
    of 2^1 rows is only 8-byte aligned and the commit transforms and hashes them there.  The root equals the oracle session's commit of
    the same columns, both hash modes."""
    logs, host, want = PL.session_case(mode)
    s = be.prover_session(nz.default_config(hash_mode=mode), max(logs) + 1)
    try:
        ptrs = s.tree_begin(logs)
        i = 0
        while i < len(logs):                        # one slab per run of equal sizes: column k of the run at base + (k << log)
            j = i
            while j < len(logs) and logs[j] == logs[i]:
                assert ptrs[j] == ptrs[i] + ((j - i) * 4 << logs[i]), (i, j, ptrs)
                j += 1
            assert ptrs[i] % 256 == 0
            i = j
        assert ptrs[1] % 16 == 8                    # the placement this test is about
        for ptr, h in zip(ptrs, host):
            be._chk(be.L.nx_upload(be.ctx, C.c_void_p(ptr), u32p(h), C.c_size_t(h.size)))
        assert np.array_equal(s.tree_commit(), want)
    finally:
        s.close()
