"""nexus_zkvm_amd — MI355X (gfx950) backend for the Nexus zkVM commit-and-prove hot path.

Thin ctypes mirror of include/nexus_hip.h.  The names follow the Stwo backend traits the reference
instantiates on `SimdBackend` (reference prover/src/machine.rs:16,186,203,286):
`HipBackend.precompute_twiddles`, `.interpolate_columns`, `.evaluate_polynomials`, `.commit` (Merkle),
`.eval_at_points`, `.accumulate_quotients`, `.fold_line`, `.fold_circle_into_line`, `.grind`, and the
synthetic-machine `prove`.  There is NO CPU fallback: importing works without a GPU (so the symbol
table can be checked), but creating a `HipBackend` raises if libnexus_hip.so or a gfx950 device is
missing.
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NX_LIB") or os.path.join(_HERE, "libnexus_hip.so")   # NX_LIB: A/B builds for tools/ only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "nexus_hip.h")

P = (1 << 31) - 1
NX_OK = 0
NX_ERR_PROTOCOL = -4
HASH_BLAKE2S, HASH_BLAKE2S_RAW0 = 0, 1
FRI_ALPHA_PREV, FRI_ALPHA_FIRST = 0, 1
# element kinds of the narrow host-column entry points (NX_COL_* of include/nexus_hip.h)
COL_U32, COL_U16, COL_U8, COL_U32_AS_U16, COL_U32_AS_U8 = 0, 1, 2, 3, 4


class LocalGroup:
    """nx_comm_group: the shared board of the in-process transport (one per proof; HipBackend.local_comm(group, rank) per thread)."""

    def __init__(self, world):
        self.world = int(world)
        self.h = C.c_void_p()
        L = load_library()
        rc = L.nx_comm_group_create(self.world, C.byref(self.h))
        if rc != 0:
            raise NexusHipError(f"nx_comm_group_create failed ({rc}): {L.nx_last_error(None).decode()}")

    def reset(self):
        """Re-arm a group a failure broke (nx_comm_group_reset): only when every rank's thread has left its prove call."""
        L = load_library()
        rc = L.nx_comm_group_reset(self.h)
        if rc != 0:
            raise NexusHipError(f"nx_comm_group_reset failed ({rc}): {L.nx_last_error(None).decode()}")

    def broken(self):
        return bool(load_library().nx_comm_group_broken(self.h))

    def peer_access(self, from_rank, to_rank):
        """1 peer to peer / same device, 0 staged by the runtime, -1 a communicator does not exist yet (nx_comm_group_peer_access)"""
        return int(load_library().nx_comm_group_peer_access(self.h, int(from_rank), int(to_rank)))

    def close(self):
        if self.h:
            load_library().nx_comm_group_destroy(self.h)
            self.h = C.c_void_p()


class NexusHipError(RuntimeError):
    pass


class ComponentSpec(C.Structure):
    _fields_ = [("log_size", C.c_uint32), ("n_pre", C.c_uint32), ("n_main", C.c_uint32), ("n_inter", C.c_uint32),
                ("log_constraint_degree_bound", C.c_uint32),   # 0 = the config's log_constraint_degree
                ("logup_mode", C.c_uint32)]                    # nx_prove_machine: LOGUP_PAIRS | LOGUP_ODD | LOGUP_TABLE (0: one fraction per column)


LOGUP_PAIRS, LOGUP_ODD, LOGUP_TABLE = 1, 2, 4                   # nx_component_spec.logup_mode (include/nexus_hip.h NX_LOGUP_*)
TUPLES_V1, TUPLES_KECCAK, TUPLES_V2 = 1 << 4, 2 << 4, 3 << 4    # | NX_LOGUP_TUPLES(k): the reference's relation widths / entry kinds (NX_TUPLES_*)


class PcsConfig(C.Structure):
    _fields_ = [("pow_bits", C.c_uint32), ("log_blowup", C.c_uint32), ("n_queries", C.c_uint32),
                ("log_last_layer_degree_bound", C.c_uint32), ("hash_mode", C.c_uint32), ("fri_alpha_mode", C.c_uint32),
                ("log_constraint_degree", C.c_uint32)]


_SEND_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t)
_RECV_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t)
_ALLREDUCE_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_ALLGATHER_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_BROADCAST_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32)
_ALLTOALLV_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t))
_ALLGATHER_DEV_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_ABORT_T = C.CFUNCTYPE(None, C.c_void_p)


class NxComm(C.Structure):
    """nx_comm of include/nexus_hip.h: the transport callbacks of one proof on several GPUs."""
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("user", C.c_void_p), ("send", _SEND_T), ("recv", _RECV_T),
                ("allreduce_m31", _ALLREDUCE_T), ("allgather", _ALLGATHER_T), ("broadcast", _BROADCAST_T),
                ("alltoallv", _ALLTOALLV_T), ("allgather_dev", _ALLGATHER_DEV_T), ("abort", _ABORT_T)]


def make_comm(rank, world, impl):
    """Wrap a Python object with send(dst, ptr, n_words) / recv(src, ptr, n_words) / allreduce_m31(ptr, n_words) /
    allgather(bytes) -> list of bytes / broadcast(bytes_or_None, n, root) -> bytes /
    alltoallv(send_ptr, send_off, send_cnt, recv_ptr, recv_off, recv_cnt) (lists of `world` word counts) /
    allgather_dev(send_ptr, n_words, recv_ptr) into an NxComm.  Exceptions become a non-zero return code (the library then fails
    the prove with NX_ERR_HIP)."""
    def guard(f):
        def g(*a):
            try:
                f(*a)
                return 0
            except Exception:   # noqa: BLE001 — must not unwind through C
                import traceback
                traceback.print_exc()
                return 1
        return g

    def _allgather(_u, h_send, nbytes, h_recv):
        parts = impl.allgather(C.string_at(h_send, nbytes))
        C.memmove(h_recv, b"".join(parts), nbytes * world)

    def _broadcast(_u, h_buf, nbytes, root):
        data = impl.broadcast(C.string_at(h_buf, nbytes) if rank == root else None, nbytes, root)
        C.memmove(h_buf, data, nbytes)

    def _alltoallv(_u, sp, soff, scnt, rp, roff, rcnt):
        impl.alltoallv(sp or 0, [soff[i] for i in range(world)], [scnt[i] for i in range(world)], rp or 0, [roff[i] for i in range(world)], [rcnt[i] for i in range(world)])

    def _abort():
        """nx_comm.abort: this rank's prove failed; make the peers' collectives fail instead of waiting (optional on the Python side)"""
        try:
            if hasattr(impl, "abort"):
                impl.abort()
        except Exception:   # noqa: BLE001 — must not unwind through C
            pass

    c = NxComm(rank, world, None, _SEND_T(guard(lambda _u, dst, p, n: impl.send(dst, p, n))), _RECV_T(guard(lambda _u, src, p, n: impl.recv(src, p, n))),
               _ALLREDUCE_T(guard(lambda _u, p, n: impl.allreduce_m31(p, n))), _ALLGATHER_T(guard(_allgather)), _BROADCAST_T(guard(_broadcast)),
               _ALLTOALLV_T(guard(_alltoallv)), _ALLGATHER_DEV_T(guard(lambda _u, sp, n, rp: impl.allgather_dev(sp or 0, n, rp or 0))),
               _ABORT_T(lambda _u: _abort()))
    c._impl = impl   # keep the callbacks' target alive
    return c


def rccl_unique_id():
    """ncclGetUniqueId through the library's native RCCL transport (rank 0 calls it and ships the 128 bytes to the other ranks)."""
    L = load_library()
    buf = (C.c_uint8 * 128)()
    rc = L.nx_rccl_unique_id(buf)
    if rc != 0:
        raise NexusHipError(f"nx_rccl_unique_id failed ({rc}): {L.nx_last_error(None).decode()}")
    return bytes(buf)


def _select_arg(select, n_c):
    if select is None:
        return None, None
    sel = np.ascontiguousarray(np.asarray(select, dtype=np.uint8).reshape(-1))
    assert len(sel) == n_c, "one flag per constraint"
    return sel, sel.ctypes.data_as(C.c_void_p)


def air_source(program, n_cols, select=None):
    """The HIP source nx_air_compile(_subset) generates for a recorded program (needs no GPU and no context).
    select: one flag per constraint (None = all)."""
    L = load_library()
    ins = _u32(program.instrs).reshape(-1)
    n_c = int(sum(1 for op in ins[0::4] if op in (13, 14)))
    src = C.c_void_p()
    sel, sel_p = _select_arg(select, n_c)
    rc = L.nx_air_compile_subset(None, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, n_cols, len(_u32(program.econsts).reshape(-1)) // 4, n_c, sel_p,
                                 None, C.byref(src))
    if rc != 0:
        raise NexusHipError(f"nx_air_compile failed ({rc}): {L.nx_last_error(None).decode()}")
    try:
        return C.string_at(src.value).decode()
    finally:
        L.nx_free_host(src)


def logup_program_source(program, n_cols, n_logup_cols):
    """The HIP source nx_logup_program generates for a fraction program (needs no GPU and no context)."""
    L = load_library()
    ins = _u32(program.instrs).reshape(-1)
    ec = _u32(program.econsts).reshape(-1)
    src = C.c_char_p()
    rc = L.nx_logup_program(None, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, None, n_cols, ec.ctypes.data_as(C.c_void_p) if len(ec) else None, len(ec) // 4,
                            4, n_logup_cols, None, C.byref(src))
    if rc != 0:
        raise NexusHipError(f"nx_logup_program failed ({rc}): {L.nx_last_error(None).decode()}")
    out = src.value.decode()
    L.nx_free_host(src)
    return out


def trace_program_source(program, n_cols):
    """The HIP source nx_trace_program generates for a trace program, ProgramBuilder.build_trace_program() (needs no GPU and no context)."""
    L = load_library()
    ins = _u32(program.instrs).reshape(-1)
    src = C.c_void_p()
    rc = L.nx_trace_program(None, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, None, n_cols, 4, C.byref(src))
    if rc != 0:
        raise NexusHipError(f"nx_trace_program failed ({rc}): {L.nx_last_error(None).decode()}")
    try:
        return C.string_at(src.value).decode()
    finally:
        L.nx_free_host(src)


def air_check_source(program, n_cols):
    """The HIP source of the check kernels nx_air_check compiles for a recorded program (needs no GPU and no context)."""
    L = load_library()
    ins = _u32(program.instrs).reshape(-1)
    n_c = int(sum(1 for op in ins[0::4] if op in (13, 14)))
    src = C.c_void_p()
    rc = L.nx_air_check_source(ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, n_cols, len(_u32(program.econsts).reshape(-1)) // 4, n_c, C.byref(src))
    if rc != 0:
        raise NexusHipError(f"nx_air_check_source failed ({rc}): {L.nx_last_error(None).decode()}")
    try:
        return C.string_at(src.value).decode()
    finally:
        L.nx_free_host(src)


class CheckFailureC(C.Structure):
    _fields_ = [("component", C.c_uint32), ("constraint", C.c_uint32), ("first_row", C.c_uint32), ("value", C.c_uint32 * 4), ("n_rows", C.c_uint64)]


class CheckFailure(collections.namedtuple("CheckFailure", "component constraint first_row value n_rows")):
    """One failing constraint of a trace check (nx_check_failure): first_row is a natural trace row, value a 4-tuple."""


class CheckReport:
    """What nx_air_check / nx_prover_check found: ok, n_failed (all failing constraints), failures (the first max_failures of them, in
    (component, constraint) order) and message (nx_last_error's sentence about the first one, "" when ok)."""

    def __init__(self, n_failed, failures, message):
        self.n_failed, self.failures, self.message = n_failed, failures, message
        self.ok = n_failed == 0

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return f"CheckReport(ok={self.ok}, n_failed={self.n_failed}, failures={self.failures!r})"


def _check_report(be, rc, arr, n_failed, cap):
    if rc not in (0, -4):        # NX_OK / NX_ERR_PROTOCOL: both carry a report
        be._chk(rc)
    fl = [CheckFailure(int(f.component), int(f.constraint), int(f.first_row), tuple(int(v) for v in f.value), int(f.n_rows)) for f in arr[:min(cap, n_failed.value)]]
    return CheckReport(int(n_failed.value), fl, be.L.nx_last_error(be.ctx).decode() if rc else "")


def air_constraint_degrees(program, n_cols):
    """nx_air_constraint_degrees: an upper bound of every constraint's degree in the trace columns (host only)."""
    L = load_library()
    ins = _u32(program.instrs).reshape(-1)
    n_c = int(sum(1 for op in ins[0::4] if op in (13, 14)))
    out = np.zeros(max(1, n_c), np.uint32)
    rc = L.nx_air_constraint_degrees(None, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, n_cols, len(_u32(program.econsts).reshape(-1)) // 4, n_c,
                                     out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise NexusHipError(f"nx_air_constraint_degrees failed ({rc}): {L.nx_last_error(None).decode()}")
    return out[:n_c]


def air_cache_dir(path):
    """nx_air_cache_dir: the directory the library keeps compiled AIR kernels in (None = off).  Process-wide."""
    L = load_library()
    rc = L.nx_air_cache_dir(path.encode() if path else None)
    if rc != 0:
        raise NexusHipError(f"nx_air_cache_dir failed ({rc})")


def air_cache_stats():
    """(kernels compiled by hiprtc, loaded from the cache directory, stored into it) by this process"""
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    load_library().nx_air_cache_stats(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)


class AirKernel:
    """A recorded AIR compiled by hiprtc (nx_air_compile / nx_air_compile_subset); eval() matches HipBackend.eval_constraint_program.
    select: one flag per constraint — the kernel evaluates only those (columns they do not read may be passed as None to eval)."""

    def __init__(self, be, program, n_cols, select=None, blob=None):
        """blob: a kernel saved by save() (nx_air_kernel_load: no compilation) — the program is still needed for eval()'s default constants"""
        self.be, self.program, self.n_cols = be, program, n_cols
        ins = _u32(program.instrs).reshape(-1)
        self.n_constraints = int(sum(1 for op in ins[0::4] if op in (13, 14)))
        self.h = C.c_void_p()
        if blob is not None:
            b = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
            be._chk(be.L.nx_air_kernel_load(be.ctx, b, C.c_size_t(len(blob)), C.byref(self.h)))
            return
        sel, sel_p = _select_arg(select, self.n_constraints)
        be._chk(be.L.nx_air_compile_subset(be.ctx, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, n_cols, len(_u32(program.econsts).reshape(-1)) // 4,
                                           self.n_constraints, sel_p, C.byref(self.h), None))

    def save(self):
        """The compiled kernel as bytes (nx_air_kernel_save): header + gfx950 code object, loadable by AirKernel(..., blob=...)."""
        p, n = C.c_void_p(), C.c_size_t()
        self.be._chk(self.be.L.nx_air_kernel_save(self.h, C.byref(p), C.byref(n)))
        out = C.string_at(p, n.value)
        self.be.L.nx_free_host(p)
        return out

    def eval(self, column_ptrs, alpha_powers, denom_inv, log_size, log_eval, acc4, econsts=None):
        assert len(column_ptrs) == self.n_cols
        ptrs = (C.c_void_p * max(1, len(column_ptrs)))(*column_ptrs)
        ec = _u32(self.program.econsts if econsts is None else econsts).reshape(-1)
        pw = _u32(alpha_powers).reshape(-1)
        assert len(pw) // 4 == self.n_constraints
        den = _u32(denom_inv)
        assert len(den) == 1 << (log_eval - log_size)
        self.be._chk(self.be.L.nx_air_eval(self.be.ctx, self.h, ptrs, ec.ctypes.data_as(C.c_void_p), pw.ctypes.data_as(C.c_void_p), den.ctypes.data_as(C.c_void_p),
                                           log_size, log_eval, acc4.col_ptrs()))
        return acc4

    def close(self):
        if self.h and self.be.ctx:
            self.be.L.nx_air_kernel_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AirComponentC(C.Structure):
    _fields_ = [("log_size", C.c_uint32), ("program", C.c_void_p), ("n_instr", C.c_uint32), ("n_regs", C.c_uint32), ("econsts", C.c_void_p),
                ("n_econsts", C.c_uint32), ("n_constraints", C.c_uint32), ("col_tree", C.c_void_p), ("col_index", C.c_void_p), ("n_cols", C.c_uint32),
                ("mask_count", C.c_void_p), ("mask_offsets", C.c_void_p), ("kernel", C.c_void_p), ("log_constraint_degree_bound", C.c_uint32)]


def _air_components(components, kernels=None):
    """air_program.Component list -> the nx_air_component array of nx_prover_prove / nx_verifier_verify (and the arrays it points into)."""
    arr = (AirComponentC * len(components))()
    keep = []
    for i, c in enumerate(components):
        pr = c.program
        ins, ec = _u32(pr.instrs).reshape(-1), _u32(pr.econsts).reshape(-1)
        ct, ci = _u32([t for t, _ in c.cols]), _u32([k for _, k in c.cols])
        mc = _u32([len(m) for m in c.masks])
        mo = np.ascontiguousarray([o for m in c.masks for o in m], dtype=np.int32)
        keep += [ins, ec, ct, ci, mc, mo]
        a = arr[i]
        a.log_size, a.program, a.n_instr, a.n_regs = c.log_size, ins.ctypes.data, len(ins) // 4, pr.n_regs
        a.econsts, a.n_econsts, a.n_constraints = ec.ctypes.data if len(ec) else None, len(ec) // 4, pr.n_constraints
        a.col_tree, a.col_index, a.n_cols = ct.ctypes.data if len(ct) else None, ci.ctypes.data if len(ci) else None, len(c.cols)
        a.mask_count, a.mask_offsets = mc.ctypes.data if len(mc) else None, mo.ctypes.data if len(mo) else None
        a.kernel = kernels[i].h if kernels else None
        a.log_constraint_degree_bound = getattr(c, "log_constraint_degree_bound", 0)
    return arr, keep


class ProverSession:
    """nx_prover_*: CommitmentSchemeProver + Blake2sChannel + stwo::prover::prove over recorded AIRs
    (air_program.Component).  The caller drives the reference's transcript prefix (machine.rs:198-263)."""

    def __init__(self, be, cfg, max_log_size):
        self.be, self.cfg = be, cfg
        self.h = C.c_void_p()
        be._chk(be.L.nx_prover_create(be.ctx, C.byref(cfg), max_log_size, C.byref(self.h)))

    def set_comm(self, comm):
        """ONE proof on several GPUs: every rank runs the same session calls; tree_begin then returns None for the columns of
        other ranks (nx_prover_set_comm).  Call before the first tree."""
        self._comm = comm
        self.be._chk(self.be.L.nx_prover_set_comm(self.h, C.byref(comm)))

    def mix_u64(self, v):
        self.be._chk(self.be.L.nx_prover_mix_u64(self.h, C.c_uint64(int(v))))

    def mix_felts(self, felts):
        f = _u32(felts).reshape(-1)
        self.be._chk(self.be.L.nx_prover_mix_felts(self.h, f.ctypes.data_as(C.c_void_p), len(f) // 4))

    def draw_felt(self):
        out = np.zeros(4, np.uint32)
        self.be._chk(self.be.L.nx_prover_draw_felt(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def draw_felts(self, n):
        out = np.zeros((n, 4), np.uint32)
        self.be._chk(self.be.L.nx_prover_draw_felts(self.h, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def digest(self):
        out = np.zeros(8, np.uint32)
        self.be._chk(self.be.L.nx_prover_channel_digest(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def tree_begin(self, log_sizes):
        """Device addresses (ints) of the next tree's columns, to be filled with bit-reversed circle-domain evaluations."""
        logs = _u32(log_sizes)
        ptrs = (C.c_void_p * max(1, len(logs)))()
        self.be._chk(self.be.L.nx_prover_tree_begin(self.h, logs.ctypes.data_as(C.c_void_p), len(logs), ptrs))
        return [int(ptrs[i] or 0) for i in range(len(logs))]

    def tree_commit(self):
        root = np.zeros(8, np.uint32)
        self.be._chk(self.be.L.nx_prover_tree_commit(self.h, root.ctypes.data_as(C.c_void_p)))
        return root

    def commit(self, cols):
        """Host columns (numpy, bit-reversed circle-domain evaluations): tree_begin + upload + tree_commit; returns the root."""
        cols = [_u32(c) for c in cols]
        ptrs = self.tree_begin([int(np.log2(len(c))) for c in cols])
        for c, d in zip(cols, ptrs):
            if d:        # row-sharded prove: only this rank's columns are handed out
                self.be._chk(self.be.L.nx_upload(self.be.ctx, C.c_void_p(d), c.ctypes.data_as(C.c_void_p), C.c_size_t(len(c))))
        return self.tree_commit()

    def commit_host(self, cols, coset_order=False, keep=()):
        """nx_prover_tree_commit_host: the tree's columns stay in HOST memory (numpy) and are uploaded chunk by chunk under the commit's
        own transforms.  keep: column indices whose evaluations are cloned on arrival; returns (root, {index: DeviceColumns})."""
        return self._commit_host([_u32(c) for c in cols], None, coset_order, keep)

    def commit_host_narrow(self, cols, coset_order=False, keep=(), as_kind=None):
        """nx_prover_tree_commit_host_narrow: commit_host for host columns of uint8 / uint16 / uint32 arrays (the kind follows the dtype;
        as_kind declares uint32 columns to hold byte or half-word values, see _narrow_columns).  Narrow columns cross PCIe narrow and are
        widened on the device.  A value that does not fit its declared width raises; the tree is then no longer begun and the transcript
        is untouched.  Returns (root, {index: DeviceColumns})."""
        arrs, kinds = _narrow_columns(cols, as_kind)
        return self._commit_host(arrs, kinds, coset_order, keep)

    def _commit_host(self, arrs, kinds, coset_order, keep):
        """commit_host (kinds None: nx_prover_tree_commit_host) and commit_host_narrow (nx_prover_tree_commit_host_narrow)."""
        L = self.be.L
        fn = L.nx_prover_tree_commit_host if kinds is None else L.nx_prover_tree_commit_host_narrow
        logs = [int(np.log2(len(c))) for c in arrs]
        self.tree_begin(logs)
        kept = {int(k): DeviceColumns(self.be, 1, logs[int(k)]) for k in keep}
        ki = _u32(list(kept.keys()))
        kd = (C.c_void_p * max(1, len(kept)))(*[d.ptr.value for d in kept.values()])
        root = np.zeros(8, np.uint32)
        self.be._chk(fn(self.h, *_host_columns(arrs, kinds), int(bool(coset_order)), ki.ctypes.data_as(C.c_void_p) if len(kept) else None, len(kept),
                        kd if len(kept) else None, root.ctypes.data_as(C.c_void_p)))
        return root, kept

    def share_tree(self, tree_index):
        """nx_prover_tree_share: committed tree `tree_index` of this session as a handle other sessions of the same backend can adopt."""
        h = C.c_void_p()
        self.be._chk(self.be.L.nx_prover_tree_share(self.h, int(tree_index), C.byref(h)))
        return SharedTree(self.be, h)

    def adopt_tree(self, shared):
        """nx_prover_tree_adopt: the shared tree becomes this session's next tree (no upload, no transform, no hashing); returns the root."""
        root = np.zeros(8, np.uint32)
        self.be._chk(self.be.L.nx_prover_tree_adopt(self.h, shared.h, root.ctypes.data_as(C.c_void_p)))
        return root

    def prove(self, components, kernels=None, want_stats=False):
        """components: air_program.Component list; kernels: optional AirKernel per component (compiled once, reused)."""
        arr, keep = _air_components(components, kernels)
        words, n = C.POINTER(C.c_uint32)(), C.c_size_t(0)
        stats = ProveStats()
        self.be._chk(self.be.L.nx_prover_prove(self.h, arr, len(components), C.byref(words), C.byref(n), C.byref(stats) if want_stats else None))
        out = np.ctypeslib.as_array(words, shape=(n.value,)).copy()
        self.be.L.nx_free_host(words)
        return (out, stats.as_dict()) if want_stats else out

    def check(self, components, max_failures=64):
        """nx_prover_check: every recorded constraint of every component on every row of its trace domain (the committed trees); a
        CheckReport instead of an exception when constraints fail.  Leaves the transcript and later proofs alone."""
        arr, keep = _air_components(components)
        out = (CheckFailureC * max(1, max_failures))()
        n = C.c_uint32(0)
        rc = self.be.L.nx_prover_check(self.h, arr, len(components), out, int(max_failures), C.byref(n))
        return _check_report(self.be, rc, out, n, max_failures)

    def close(self):
        if self.h and self.be.ctx:
            self.be.L.nx_prover_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SharedTree:
    """A committed tree shared between sessions (nx_committed_tree): release() when no further session will adopt it."""

    def __init__(self, be, h):
        self.be, self.h = be, h

    def root(self):
        r, n = np.zeros(8, np.uint32), C.c_uint32()
        self.be._chk(self.be.L.nx_committed_tree_root(self.h, r.ctypes.data_as(C.c_void_p), C.byref(n)))
        return r, int(n.value)

    def release(self):
        if self.h and self.be.ctx:
            self.be.L.nx_committed_tree_release(self.h)
        self.h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


NX_ERR_ARG, NX_ERR_VERIFY = -2, -6


class VerifierSession:
    """nx_verifier_*: CommitmentSchemeVerifier + Blake2sChannel + core::verifier::verify over recorded AIRs, the mirror of ProverSession
    (reference prover/src/machine.rs:299-485).  Host only: needs no HipBackend and no GPU.  hash_mode: the node-hash rule (default: the
    config's)."""

    def __init__(self, cfg, hash_mode=None):
        self.L, self.cfg = load_library(), cfg
        self.h = C.c_void_p()
        rc = self.L.nx_verifier_create(C.byref(cfg), int(cfg.hash_mode if hash_mode is None else hash_mode), C.byref(self.h))
        if rc != NX_OK:
            raise NexusHipError(f"nx_verifier_create failed (rc={rc}): configuration outside the verifier's range")

    def _chk(self, rc):
        if rc != NX_OK:
            raise NexusHipError(f"libnexus_hip verifier error {rc}: {self.last_error()}")

    def last_error(self):
        return self.L.nx_verifier_last_error(self.h).decode()

    def mix_u64(self, v):
        self._chk(self.L.nx_verifier_mix_u64(self.h, C.c_uint64(int(v))))

    def mix_felts(self, felts):
        f = _u32(felts).reshape(-1)
        self._chk(self.L.nx_verifier_mix_felts(self.h, f.ctypes.data_as(C.c_void_p), len(f) // 4))

    def draw_felt(self):
        out = np.zeros(4, np.uint32)
        self._chk(self.L.nx_verifier_draw_felt(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def draw_felts(self, n):
        out = np.zeros((n, 4), np.uint32)
        self._chk(self.L.nx_verifier_draw_felts(self.h, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def digest(self):
        out = np.zeros(8, np.uint32)
        self._chk(self.L.nx_verifier_channel_digest(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def commit(self, root, log_sizes):
        """CommitmentSchemeVerifier::commit: the root (8 words) of the next tree and its columns' trace log sizes."""
        r, logs = _u32(root), _u32(log_sizes)
        self._chk(self.L.nx_verifier_tree_commit(self.h, r.ctypes.data_as(C.c_void_p), logs.ctypes.data_as(C.c_void_p), len(logs)))

    def commit_columns(self, be, tw, column_sets):
        """The same with the root computed from device columns (HipBackend.commit_root; the columns are consumed).  Returns the root."""
        ptrs, logs = [], []
        for s in column_sets:
            ptrs += [s.ptr.value + i * (4 << s.log_size) for i in range(s.n_cols)]
            logs += [s.log_size] * s.n_cols
        arr, lg, root = (C.c_void_p * max(1, len(ptrs)))(*ptrs), _u32(logs), np.zeros(8, np.uint32)
        rc = self.L.nx_verifier_tree_commit_columns(self.h, be.ctx, tw.h, arr, lg.ctypes.data_as(C.c_void_p), len(logs), root.ctypes.data_as(C.c_void_p))
        if rc != NX_OK:
            raise NexusHipError(f"nx_verifier_tree_commit_columns failed (rc={rc}): {self.last_error() or be.L.nx_last_error(be.ctx).decode()}")
        return root

    def verify(self, components, words):
        """None when the proof is accepted, else the text of the failing check (self.rc: NX_ERR_VERIFY or NX_ERR_ARG)."""
        arr, keep = _air_components(components)
        w = _u32(words)
        self.rc = self.L.nx_verifier_verify(self.h, arr, len(components), w.ctypes.data_as(C.c_void_p), C.c_size_t(len(w)))
        del keep
        return None if self.rc == NX_OK else self.last_error()

    def close(self):
        if self.h:
            self.L.nx_verifier_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _comp_specs(comps):
    return (ComponentSpec * len(comps))(*[ComponentSpec(*[int(x) for x in c]) for c in comps])


def verify_synth(comps, cfg, words, ad=b"", hash_mode=None, want_rc=False):
    """nx_verify_synth — `nexus_vm_prover::verify` for the synthetic machine of HipBackend.prove.  Host only.  None when accepted, else
    the failing check; want_rc: (text or None, return code)."""
    L = load_library()
    w, err = _u32(words), C.create_string_buffer(512)
    adb = (C.c_uint8 * max(1, len(ad)))(*ad)
    rc = L.nx_verify_synth(_comp_specs(comps), len(comps), C.byref(cfg), int(cfg.hash_mode if hash_mode is None else hash_mode), adb, C.c_size_t(len(ad)),
                           w.ctypes.data_as(C.c_void_p), C.c_size_t(len(w)), err, C.c_size_t(len(err)))
    text = None if rc == NX_OK else (err.value.decode() or f"error {rc}")
    return (text, rc) if want_rc else text


def verify_machine(comps, cfg, words, claimed_sums, ad=b"", hash_mode=None, expected_logup_sum=None, want_rc=False):
    """nx_verify_machine — `nexus_vm_prover::verify` for the machine of HipBackend.prove_machine; claimed_sums: (n_components, 4) words
    (HipBackend.machine_claimed_sums); expected_logup_sum: 4 words the claimed sums must add up to, or None for no such check.
    Host only.  None when accepted, else the failing check."""
    L = load_library()
    w, err = _u32(words), C.create_string_buffer(512)
    cs = _u32(claimed_sums).reshape(-1)
    if len(cs) != 4 * len(comps):
        raise ValueError("claimed_sums: 4 words per component")
    ex = _u32(expected_logup_sum).reshape(4) if expected_logup_sum is not None else None
    adb = (C.c_uint8 * max(1, len(ad)))(*ad)
    rc = L.nx_verify_machine(_comp_specs(comps), len(comps), C.byref(cfg), int(cfg.hash_mode if hash_mode is None else hash_mode), adb, C.c_size_t(len(ad)),
                             w.ctypes.data_as(C.c_void_p), C.c_size_t(len(w)), cs.ctypes.data_as(C.c_void_p),
                             ex.ctypes.data_as(C.c_void_p) if ex is not None else None, err, C.c_size_t(len(err)))
    text = None if rc == NX_OK else (err.value.decode() or f"error {rc}")
    return (text, rc) if want_rc else text


class LogupFrac(C.Structure):
    """nx_logup_frac of include/nexus_hip.h."""
    _fields_ = [("d_tuple_cols", C.c_void_p), ("n_tuple_cols", C.c_uint32), ("alpha_powers", C.c_void_p), ("z", C.c_void_p), ("d_mult", C.c_void_p),
                ("scale", C.c_void_p)]


class LookupUse(C.Structure):
    """nx_lookup_use of include/nexus_hip.h."""
    _fields_ = [("d_values", C.c_void_p), ("d_weight", C.c_void_p), ("log_size", C.c_uint32)]


CHAIN_GIVEN, CHAIN_ADD, CHAIN_BYTES = 0, 1, 2     # NX_CHAIN_* of include/nexus_hip.h


class AccessStream(C.Structure):
    """nx_access_stream of include/nexus_hip.h."""
    _fields_ = [("d_key", C.c_void_p), ("d_flag", C.c_void_p), ("d_payload", C.c_void_p), ("d_prev", C.c_void_p), ("d_ordinal", C.c_void_p),
                ("log_size", C.c_uint32), ("epoch", C.c_uint32), ("linear", C.c_uint32)]


class AccessSummary(C.Structure):
    """nx_access_summary of include/nexus_hip.h."""
    _fields_ = [("cap", C.c_uint32), ("d_key", C.c_void_p), ("d_count", C.c_void_p), ("d_last", C.c_void_p)]


class ChainStream(C.Structure):
    """nx_chain_stream of include/nexus_hip.h."""
    _fields_ = [("d_key", C.c_void_p), ("d_flag", C.c_void_p), ("d_row", C.c_void_p), ("d_payload", C.c_void_p), ("rule", C.c_void_p), ("delta", C.c_void_p),
                ("d_prev", C.c_void_p), ("d_ordinal", C.c_void_p), ("log_size", C.c_uint32), ("n_records", C.c_uint32), ("span", C.c_uint32), ("epoch", C.c_uint32),
                ("linear", C.c_uint32)]


class PartLimb(C.Structure):
    """nx_part_limb of include/nexus_hip.h."""
    _fields_ = [("src", C.c_uint32), ("shift", C.c_uint32), ("bits", C.c_uint32)]


class PartDest(C.Structure):
    """nx_part_dest of include/nexus_hip.h."""
    _fields_ = [("cls", C.c_uint32), ("log_size", C.c_uint32), ("n_cols", C.c_uint32), ("d_cols", C.c_void_p), ("limbs", C.c_void_p), ("d_is_pad", C.c_void_p),
                ("d_step", C.c_void_p)]


PART_NONE = PART_ALL = 0xFFFFFFFF   # NX_PART_NONE (a class word), NX_PART_ALL (a destination's class)
PART_MAX_CLASSES = 256              # NX_PART_MAX_CLASSES


def partition_log_size(count, min_log):
    """nx_trace_partition_log_size: max(ceil_log2(count), min_log), the log_size of a component with `count` steps.  Host only."""
    L = load_library()
    L.nx_trace_partition_log_size.restype = C.c_uint32
    L.nx_trace_partition_log_size.argtypes = [C.c_uint64, C.c_uint32]
    return int(L.nx_trace_partition_log_size(int(count), int(min_log)))


class TracePartition:
    """The stable order of a step table by class (nx_partition), from HipBackend.trace_partition.  counts: steps per class."""

    def __init__(self, backend, handle, counts, n_steps):
        self.be, self.h, self.counts, self.n_steps = backend, handle, counts, n_steps

    def fill(self, src_ptrs, dests, want_rc=False):
        """nx_trace_partition_fill: every destination (one component) from the step table in one call.  src_ptrs: device addresses of
        the table's columns, n_steps words each in step order; dests: dicts with cls (a class, or PART_ALL for every step), log_size,
        cols (device addresses of 2^log_size words, bit-reversed circle-domain order), limbs (one (src, shift, bits) per column: natural
        row r holds (src[step_r] >> shift) & (2^bits - 1)), optional is_pad / step (output addresses).  Stream-ordered.  want_rc:
        the return code instead of raising on NX_ERR_ARG."""
        keep = []
        arr = (PartDest * max(1, len(dests)))()
        for i, d in enumerate(dests):
            cols, limbs = list(d.get("cols", ())), list(d.get("limbs", ()))
            if len(cols) != len(limbs):
                raise NexusHipError(f"trace_partition fill: destination {i} has {len(cols)} columns and {len(limbs)} limb specs")
            cp = (C.c_void_p * max(1, len(cols)))(*[int(x) if x else None for x in cols])
            lp = (PartLimb * max(1, len(limbs)))(*[PartLimb(int(s), int(sh), int(b)) for s, sh, b in limbs])
            keep += [cp, lp]
            arr[i] = PartDest(int(d["cls"]), int(d["log_size"]), len(cols), C.cast(cp, C.c_void_p), C.cast(lp, C.c_void_p),
                              int(d["is_pad"]) if d.get("is_pad") else None, int(d["step"]) if d.get("step") else None)
        sp = (C.c_void_p * max(1, len(src_ptrs)))(*[int(x) if x else None for x in src_ptrs])
        rc = self.be.L.nx_trace_partition_fill(self.be.ctx, self.h, sp, C.c_uint32(len(src_ptrs)), arr, C.c_uint32(len(dests)))
        del keep
        if want_rc and rc in (NX_OK, NX_ERR_ARG):
            return rc
        self.be._chk(rc)
        return rc

    def destroy(self):
        if self.h and self.be.ctx:
            self.be.L.nx_trace_partition_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


MULT_LDS_MAX_KEY_BITS = 12   # NX_MULT_LDS_MAX_KEY_BITS: widest key space nx_logup_multiplicities counts in LDS
MULT_SPARSE_LDS_LOG_KEYS = 12   # NX_MULT_SPARSE_LDS_LOG_KEYS: largest table (log rows) nx_logup_multiplicities_sparse searches in LDS alone
KECCAK_ROUND_MAIN_COLS, KECCAK_ROUND_PRE_COLS = 1705, 9  # NX_KECCAK_ROUND_MAIN_COLS, NX_KECCAK_ROUND_PRE_COLS
KECCAK_MEMCHECK_MAIN_COLS, KECCAK_MEMCHECK_PRE_COLS = 2001, 1   # NX_KECCAK_MEMCHECK_MAIN_COLS, NX_KECCAK_MEMCHECK_PRE_COLS


class ProveStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("trace_gen", "commit", "composition", "oods", "quotients", "fri", "pow", "decommit", "total")] + \
               [("lde_kernel_ms", C.c_double), ("lde_algorithmic_bytes", C.c_uint64), ("merkle_kernel_ms", C.c_double),
                ("merkle_algorithmic_bytes", C.c_uint64), ("interaction", C.c_double), ("comm_ms", C.c_double), ("comm_bytes", C.c_uint64),
                ("n_alltoallv", C.c_uint32), ("n_allgather_dev", C.c_uint32), ("n_allgather_host", C.c_uint32), ("n_comm_reserved", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


_lib = None


def load_library():
    """Loads libnexus_hip.so (built in-tree by __graft_entry__.build / csrc/Makefile).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NexusHipError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.nx_last_error.restype = C.c_char_p
    L.nx_last_error.argtypes = [C.c_void_p]
    L.nx_version.restype = C.c_char_p
    L.nx_ctx_stream.restype = C.c_void_p
    L.nx_merkle_layer.restype = C.c_void_p
    L.nx_merkle_n_layers.restype = C.c_uint32
    L.nx_free_host.argtypes = [C.c_void_p]
    L.nx_air_kernel_destroy.argtypes = [C.c_void_p]
    L.nx_prover_destroy.argtypes = [C.c_void_p]
    L.nx_comm_group_destroy.argtypes = [C.c_void_p]
    L.nx_comm_local_destroy.argtypes = [C.c_void_p]
    L.nx_committed_tree_release.argtypes = [C.c_void_p]
    L.nx_committed_tree_release.restype = None
    L.nx_verifier_destroy.argtypes = [C.c_void_p]
    L.nx_trace_partition_destroy.argtypes = [C.c_void_p]
    L.nx_trace_partition_destroy.restype = None
    L.nx_verifier_destroy.restype = None
    L.nx_verifier_last_error.argtypes = [C.c_void_p]
    L.nx_verifier_last_error.restype = C.c_char_p
    for name in ("nx_ctx_destroy", "nx_twiddles_destroy", "nx_tree_destroy", "nx_free_host", "nx_air_kernel_destroy", "nx_prover_destroy", "nx_comm_group_destroy",
                 "nx_comm_local_destroy", "nx_comm_rccl_destroy"):
        getattr(L, name).restype = None
    _lib = L
    return L


def declared_symbols():
    """Function names declared in include/nexus_hip.h (used by the CPU test that the .so exports them all)."""
    import re
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nx_[a-z0-9_]+)\s*\(", text)))


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _as_width(spec):
    """A narrower width for a uint32 column: np.uint8 / np.uint16 (or "u8" / "u16"); None keeps it uint32."""
    if spec is None:
        return None
    name = spec if isinstance(spec, str) else np.dtype(spec).name
    w = {"u8": 1, "uint8": 1, "u16": 2, "uint16": 2}.get(name)
    if w is None:
        raise ValueError(f"as_kind: {spec!r} is not a narrower width (uint8 / uint16)")
    return w


def _narrow_columns(cols, as_kind=None):
    """Host columns of the narrow entry points -> (contiguous arrays to keep alive, their NX_COL_* kinds as a uint8 array).  The kind
    follows the dtype (uint8 / uint16 / uint32); as_kind (one spec for every uint32 column, or one per column, None = as it is) declares a
    uint32 column's values to fit 1 or 2 bytes: the library packs it on host threads and refuses a value that does not fit."""
    cols = list(cols)
    per = list(as_kind) if isinstance(as_kind, (list, tuple)) else [as_kind] * len(cols)
    if len(per) != len(cols):
        raise ValueError("as_kind: one entry per column")
    arrs, kinds = [], []
    for c, spec in zip(cols, per):
        a = np.asarray(c)
        if a.dtype in (np.uint8, np.uint16):
            if spec is not None:
                raise ValueError("as_kind applies to uint32 columns only")
            arrs.append(np.ascontiguousarray(a)); kinds.append(COL_U8 if a.dtype == np.uint8 else COL_U16)
            continue
        arrs.append(_u32(a))
        w = _as_width(spec)
        kinds.append(COL_U32 if w is None else COL_U32_AS_U8 if w == 1 else COL_U32_AS_U16)
    return arrs, np.array(kinds, dtype=np.uint8)


def _host_columns(arrs, kinds):
    """The arguments a host-column entry point takes for its columns: the pointer table of `arrs` and — for the narrow form (kinds not
    None) — their NX_COL_* kinds right behind it."""
    hp = (C.c_void_p * max(1, len(arrs)))(*[c.ctypes.data for c in arrs])
    return (hp,) if kinds is None else (hp, kinds.ctypes.data_as(C.c_void_p))


def default_config(pow_bits=10, log_blowup=1, n_queries=3, log_last_layer_degree_bound=0, hash_mode=HASH_BLAKE2S,
                   fri_alpha_mode=FRI_ALPHA_PREV, log_constraint_degree=1):
    """PcsConfig::default() of the pinned Stwo is unverifiable here (pow_bits 5 or 10)."""
    return PcsConfig(pow_bits, log_blowup, n_queries, log_last_layer_degree_bound, hash_mode, fri_alpha_mode, log_constraint_degree)


class DeviceColumns:
    """n_cols contiguous device columns of 2^log_size u32 words (a slab)."""

    def __init__(self, backend, n_cols, log_size):
        self.be, self.n_cols, self.log_size = backend, n_cols, log_size
        self.ptr = C.c_void_p()
        backend._chk(backend.L.nx_alloc(backend.ctx, C.c_size_t(max(1, n_cols << log_size)), C.byref(self.ptr)))

    @classmethod
    def view(cls, backend, ptr, n_cols, log_size):
        """A non-owning view of n_cols contiguous columns that live elsewhere (e.g. in a ProverSession tree)."""
        v = cls.__new__(cls)
        v.be, v.n_cols, v.log_size, v.ptr, v.borrowed = backend, n_cols, log_size, C.c_void_p(int(ptr)), True
        return v

    def col_ptrs(self):
        stride = 4 << self.log_size
        return (C.c_void_p * max(1, self.n_cols))(*[self.ptr.value + i * stride for i in range(self.n_cols)])

    def upload(self, arr2d):
        a = _u32(arr2d).reshape(self.n_cols, 1 << self.log_size)
        self.be._chk(self.be.L.nx_upload(self.be.ctx, self.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.size)))
        return self

    def to_cpu(self):
        out = np.empty((self.n_cols, 1 << self.log_size), np.uint32)
        if out.size:
            self.be._chk(self.be.L.nx_download(self.be.ctx, out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.size)))
        return out

    def free(self):
        if getattr(self, "borrowed", False):
            self.ptr = C.c_void_p()
            return
        if self.ptr and self.ptr.value:
            if self.be.ctx:   # after HipBackend.close() the context (and every allocation it cached) is gone
                self.be.L.nx_free(self.be.ctx, self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Twiddles:
    def __init__(self, backend, log_half_coset):
        self.be, self.log_half = backend, log_half_coset
        self.h = C.c_void_p()
        backend._chk(backend.L.nx_twiddles_create(backend.ctx, log_half_coset, C.byref(self.h)))

    def to_cpu(self):
        n = 1 << self.log_half
        tw, itw = np.empty(n, np.uint32), np.empty(n, np.uint32)
        self.be._chk(self.be.L.nx_twiddles_download(self.be.ctx, self.h, tw.ctypes.data_as(C.c_void_p), itw.ctypes.data_as(C.c_void_p)))
        return tw, itw

    def __del__(self):
        try:
            if self.h:
                if self.be.ctx:
                    self.be.L.nx_twiddles_destroy(self.h)
                self.h = None
        except Exception:
            pass


class MerkleTree:
    def __init__(self, backend, handle):
        self.be, self.h = backend, handle

    def root(self):
        out = np.empty(8, np.uint32)
        self.be._chk(self.be.L.nx_merkle_root(self.be.ctx, self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def layer(self, k):
        n = 8 << k
        out = np.empty(n, np.uint32)
        p = C.c_void_p(self.be.L.nx_merkle_layer(self.h, k))
        self.be._chk(self.be.L.nx_download(self.be.ctx, out.ctypes.data_as(C.c_void_p), p, C.c_size_t(n)))
        return out.reshape(-1, 8)

    def n_layers(self):
        return self.be.L.nx_merkle_n_layers(self.h)

    def __del__(self):
        try:
            if self.h:
                if self.be.ctx:
                    self.be.L.nx_tree_destroy(self.h)
                self.h = None
        except Exception:
            pass


class HipBackend:
    """One context = one GPU = one prover transcript (the reference's single &mut channel)."""

    def __init__(self, device=0):
        self.L = load_library()
        self.device = int(device)
        self.ctx = C.c_void_p()
        rc = self.L.nx_ctx_create(int(device), C.byref(self.ctx))
        if rc != NX_OK:
            raise NexusHipError(f"nx_ctx_create failed ({rc}): {self.L.nx_last_error(None).decode()}")

    def _chk(self, rc):
        if rc != NX_OK:
            raise NexusHipError(f"libnexus_hip error {rc}: {self.L.nx_last_error(self.ctx).decode()}")

    def close(self):
        if self.ctx:
            self.L.nx_ctx_destroy(self.ctx)
            self.ctx = None

    def sync(self):
        self._chk(self.L.nx_sync(self.ctx))

    def trim(self):
        """nx_ctx_trim: give the cached device blocks back to the driver (other contexts on this GPU can use them)."""
        self._chk(self.L.nx_ctx_trim(self.ctx))

    def set_hash_mode(self, mode):
        self._chk(self.L.nx_ctx_set_hash_mode(self.ctx, mode))

    def rccl_comm(self, unique_id, rank, world):
        """The native RCCL transport (csrc/comm_rccl.hip) as an NxComm for prove_machine(comm=...) / ProverSession.set_comm: no Python in
        the data path.  Free with free_rccl_comm."""
        p = C.c_void_p()
        idb = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self.L.nx_comm_rccl_create(self.ctx, idb, int(rank), int(world), C.byref(p)))
        comm = NxComm.from_address(p.value)
        comm._native = p
        return comm

    def free_rccl_comm(self, comm):
        self.L.nx_comm_rccl_destroy(comm._native)

    def local_comm(self, group, rank):
        """The in-process transport (csrc/comm_local.hip) as an NxComm: `group` = LocalGroup(world) shared by the threads of one proof,
        one thread per rank with a HipBackend of its own.  No Python in the data path.  Free with free_local_comm."""
        p = C.c_void_p()
        self._chk(self.L.nx_comm_local_create(group.h, self.ctx, int(rank), C.byref(p)))
        comm = NxComm.from_address(p.value)
        comm._native, comm._group = p, group
        return comm

    def free_local_comm(self, comm):
        self.L.nx_comm_local_destroy(comm._native)

    def set_option(self, name, value):
        """Per-context policy / tuning (nx_ctx_set_option): "fft.batch_cols", "fft.streams",
        "fri.dist_min_log", "dist.chunks", "air.segment", ...  The NX_* environment variables only seed a new context's defaults.
        The device-memory budget: "mem.limit_bytes" (0 = none; a request beyond it raises with NX_ERR_OOM, nothing left behind),
        "mem.cache_bytes" (most bytes of freed blocks kept); debug aids: "debug.fail_alloc" = n refuses the n-th following allocator
        request once; get_option("debug.alloc_count") / ("mem.cached_bytes") are read-only."""
        self._chk(self.L.nx_ctx_set_option(self.ctx, name.encode(), C.c_int64(int(value))))

    def get_option(self, name):
        v = C.c_int64()
        self._chk(self.L.nx_ctx_get_option(self.ctx, name.encode(), C.byref(v)))
        return v.value

    # ---- Column ops ----
    def clone_columns(self, cols):
        """Column::clone on device (nx_copy)."""
        out = DeviceColumns(self, cols.n_cols, cols.log_size)
        self._chk(self.L.nx_copy(self.ctx, out.ptr, cols.ptr, C.c_size_t(cols.n_cols << cols.log_size)))
        return out

    def columns(self, n_cols, log_size):
        return DeviceColumns(self, n_cols, log_size)

    def columns_from_host(self, arr2d):
        a = _u32(arr2d)
        if a.ndim == 1:
            a = a[None, :]
        return DeviceColumns(self, a.shape[0], int(np.log2(a.shape[1]))).upload(a)

    def bit_reverse_column(self, cols, index=0):
        p = C.c_void_p(cols.ptr.value + index * (4 << cols.log_size))
        self._chk(self.L.nx_bit_reverse(self.ctx, p, cols.log_size))

    def finalize_columns(self, natural):
        """R3: natural coset order -> bit-reversed circle-domain order (reference trace/utils.rs:94-106)."""
        out = DeviceColumns(self, natural.n_cols, natural.log_size)
        self._chk(self.L.nx_finalize_columns(self.ctx, natural.col_ptrs(), out.col_ptrs(), natural.n_cols, natural.log_size))
        return out

    def upload_coset_order(self, host_col):
        a = _u32(host_col)
        out = DeviceColumns(self, 1, int(np.log2(a.size)))
        self._chk(self.L.nx_upload_coset_order(self.ctx, a.ctypes.data_as(C.c_void_p), out.log_size, out.ptr))
        return out

    def upload_columns(self, host_cols, coset_order=True):
        """A whole host trace (list of 1-D uint32 arrays of one size) -> DeviceColumns, pinned in place and streamed
        (nx_upload_columns); coset_order: the host holds natural coset order (reference trace builders) and wants the
        bit-reversed circle-domain order on device."""
        return self._upload_columns([_u32(c) for c in host_cols], None, coset_order)

    def upload_columns_narrow(self, host_cols, coset_order=True, as_kind=None):
        """nx_upload_columns_narrow: upload_columns for host columns of uint8 / uint16 / uint32 arrays of one size (the kind follows the
        dtype; as_kind declares uint32 columns to hold byte or half-word values).  Narrow columns cross PCIe narrow and are widened on
        the device; a value that does not fit its declared width raises NexusHipError.  -> DeviceColumns of u32 words."""
        arrs, kinds = _narrow_columns(host_cols, as_kind)
        return self._upload_columns(arrs, kinds, coset_order)

    def _upload_columns(self, arrs, kinds, coset_order):
        """upload_columns (kinds None: nx_upload_columns) and upload_columns_narrow (nx_upload_columns_narrow)."""
        fn = self.L.nx_upload_columns if kinds is None else self.L.nx_upload_columns_narrow
        log = int(np.log2(arrs[0].size))
        out = DeviceColumns(self, len(arrs), log)
        self._chk(fn(self.ctx, *_host_columns(arrs, kinds), len(arrs), log, out.col_ptrs(), 1 if coset_order else 0))
        return out

    def host_pin(self, arr):
        """nx_host_pin: registers a contiguous host array with the driver once (a trace buffer reused across proofs); the entry points
        that take host columns then skip their own per-call pinning of it.  Undo with host_unpin before the array is freed."""
        a = np.ascontiguousarray(arr)
        if a is not arr and not np.shares_memory(a, arr):
            raise ValueError("host_pin needs a contiguous array (it pins the memory in place)")
        self._chk(self.L.nx_host_pin(self.ctx, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes)))

    def host_unpin(self, arr):
        self._chk(self.L.nx_host_unpin(self.ctx, C.c_void_p(np.ascontiguousarray(arr).ctypes.data)))

    # ---- PolyOps ----
    def precompute_twiddles(self, log_half_coset):
        return Twiddles(self, log_half_coset)

    def interpolate_columns(self, tw, cols):
        self._chk(self.L.nx_interpolate_batch(self.ctx, tw.h, cols.col_ptrs(), cols.n_cols, cols.log_size))
        return cols

    def evaluate_polynomials(self, tw, polys, log_expand):
        out = DeviceColumns(self, polys.n_cols, polys.log_size + log_expand)
        self._chk(self.L.nx_evaluate_batch(self.ctx, tw.h, polys.col_ptrs(), polys.n_cols, polys.log_size, log_expand, out.col_ptrs()))
        return out

    def lde(self, tw, cols, log_blowup):
        out = DeviceColumns(self, cols.n_cols, cols.log_size + log_blowup)
        self._chk(self.L.nx_lde_batch(self.ctx, tw.h, cols.col_ptrs(), cols.n_cols, cols.log_size, log_blowup, out.col_ptrs()))
        return out

    def lde_commit(self, tw, cols, log_blowup):
        out = DeviceColumns(self, cols.n_cols, cols.log_size + log_blowup)
        root = np.empty(8, np.uint32)
        self._chk(self.L.nx_lde_commit(self.ctx, tw.h, cols.col_ptrs(), cols.n_cols, cols.log_size, log_blowup, out.col_ptrs(),
                                       root.ctypes.data_as(C.c_void_p)))
        return out, root

    def commit_root(self, tw, column_sets, log_blowup):
        """nx_commit_root: the Merkle root of the LDE of the columns (DeviceColumns sets in commit order, mixed sizes allowed) without
        keeping the extension or the tree.  The columns are consumed (they hold coefficients afterwards)."""
        ptrs, logs = [], []
        for s in column_sets:
            ptrs += [s.ptr.value + i * (4 << s.log_size) for i in range(s.n_cols)]
            logs += [s.log_size] * s.n_cols
        arr, lg, root = (C.c_void_p * max(1, len(ptrs)))(*ptrs), _u32(logs), np.empty(8, np.uint32)
        self._chk(self.L.nx_commit_root(self.ctx, tw.h if tw is not None else None, arr, lg.ctypes.data_as(C.c_void_p), len(logs), log_blowup, root.ctypes.data_as(C.c_void_p)))
        return root

    def memory(self, reset_peak=False):
        """nx_ctx_memory: (live bytes, peak live bytes since the last reset) of the context's device allocator."""
        live, peak = C.c_uint64(), C.c_uint64()
        self._chk(self.L.nx_ctx_memory(self.ctx, C.byref(live), C.byref(peak), int(bool(reset_peak))))
        return live.value, peak.value

    def eval_at_points(self, polys, poly_idx, points):
        idx = _u32(poly_idx)
        pts = _u32(points).reshape(-1, 8)
        out = np.empty((len(idx), 4), np.uint32)
        self._chk(self.L.nx_eval_at_points(self.ctx, polys.col_ptrs(), polys.log_size, idx.ctypes.data_as(C.c_void_p),
                                           pts.ctypes.data_as(C.c_void_p), len(idx), out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- MerkleOps ----
    def merkle_commit(self, column_sets):
        """column_sets: list of DeviceColumns in commit order (mixed sizes allowed)."""
        ptrs, logs = [], []
        for cs in column_sets:
            stride = 4 << cs.log_size
            for i in range(cs.n_cols):
                ptrs.append(cs.ptr.value + i * stride)
                logs.append(cs.log_size)
        arr = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        lg = _u32(logs)
        h = C.c_void_p()
        self._chk(self.L.nx_merkle_commit(self.ctx, arr, lg.ctypes.data_as(C.c_void_p), len(ptrs), C.byref(h)))
        return MerkleTree(self, h)

    def merkle_leaf_chain(self, cols, col_offset, total_cols, state_in_ptr, state_out_ptr, row_begin=0, n_rows=None):
        """One column shard of a leaf layer (nx_merkle_leaf_chain): cols are this shard's columns (a DeviceColumns),
        state pointers are raw device addresses (ints) of n_rows x 8 words; state_in_ptr is None for the shard at column 0."""
        if n_rows is None:
            n_rows = (1 << cols.log_size) - row_begin
        self._chk(self.L.nx_merkle_leaf_chain(self.ctx, cols.col_ptrs(), cols.n_cols, cols.log_size, col_offset, total_cols,
                                              C.c_void_p(state_in_ptr) if state_in_ptr else None, C.c_void_p(state_out_ptr),
                                              C.c_uint64(row_begin), C.c_uint64(n_rows)))

    def merkle_from_leaves(self, leaf_ptr, log_size):
        """Inner layers above 2^log_size leaf digests at device address leaf_ptr (nx_merkle_from_leaves)."""
        h = C.c_void_p()
        self._chk(self.L.nx_merkle_from_leaves(self.ctx, C.c_void_p(leaf_ptr), log_size, C.byref(h)))
        return MerkleTree(self, h)


    # ---- the remaining Backend supertraits: AccumulationOps, FieldOps::batch_inverse, per-layer MerkleOps,
    #      MerkleProver::decommit, FriOps::decompose ----
    def secure_accumulate(self, dst4, src4):
        self._chk(self.L.nx_secure_accumulate(self.ctx, dst4.col_ptrs(), src4.col_ptrs(), dst4.log_size))
        return dst4

    def generate_secure_powers(self, felt, n):
        out = np.zeros((n, 4), np.uint32)
        f = _u32(felt)
        self._chk(self.L.nx_generate_secure_powers(f.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)))
        return out

    def batch_inverse_m31(self, cols):
        """Element-wise inverse of every word of a DeviceColumns (FieldOps<BaseField>::batch_inverse)."""
        out = DeviceColumns(self, cols.n_cols, cols.log_size)
        self._chk(self.L.nx_batch_inverse_m31(self.ctx, cols.ptr, out.ptr, C.c_size_t(cols.n_cols << cols.log_size)))
        return out

    def batch_inverse_qm31(self, cols4):
        out = DeviceColumns(self, 4, cols4.log_size)
        self._chk(self.L.nx_batch_inverse_qm31(self.ctx, cols4.col_ptrs(), out.col_ptrs(), C.c_size_t(1 << cols4.log_size)))
        return out

    def bit_reverse_secure(self, cols4):
        self._chk(self.L.nx_bit_reverse_secure(self.ctx, cols4.col_ptrs(), cols4.log_size))
        return cols4

    def merkle_commit_on_layer(self, log_size, prev_layer_ptr, cols):
        """One Merkle layer (MerkleOps::commit_on_layer): prev_layer_ptr = device address of the 2^(log_size+1) nodes below or None;
        cols = DeviceColumns of 2^log_size rows injected here (or None).  Returns a DeviceColumns view-like buffer of 8 * 2^log_size words."""
        out = DeviceColumns(self, 8, log_size)          # 2^log nodes x 8 words, node-major
        n = cols.n_cols if cols is not None else 0
        self._chk(self.L.nx_merkle_commit_on_layer(self.ctx, log_size, C.c_void_p(prev_layer_ptr) if prev_layer_ptr else None,
                                                   cols.col_ptrs() if n else None, n, out.ptr))
        return out

    def merkle_decommit(self, tree, column_sets, queries_per_log):
        """MerkleProver::decommit: queries_per_log = {log: sorted positions}.  Returns (queried_values, hash_witness[n, 8], column_witness)."""
        ptrs, logs = [], []
        for cs in column_sets:
            stride = 4 << cs.log_size
            for i in range(cs.n_cols):
                ptrs.append(cs.ptr.value + i * stride)
                logs.append(cs.log_size)
        arr = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        lg = _u32(logs)
        qlogs = _u32(sorted(queries_per_log))
        qcnt = _u32([len(queries_per_log[int(l)]) for l in qlogs])
        qs = np.ascontiguousarray([q for l in qlogs for q in queries_per_log[int(l)]], dtype=np.uint64)
        outs = [C.POINTER(C.c_uint32)() for _ in range(3)]
        ns = [C.c_size_t(0) for _ in range(3)]
        self._chk(self.L.nx_merkle_decommit(self.ctx, tree.h, arr, lg.ctypes.data_as(C.c_void_p), len(ptrs), qlogs.ctypes.data_as(C.c_void_p),
                                            qcnt.ctypes.data_as(C.c_void_p), len(qlogs), qs.ctypes.data_as(C.c_void_p),
                                            C.byref(outs[0]), C.byref(ns[0]), C.byref(outs[1]), C.byref(ns[1]), C.byref(outs[2]), C.byref(ns[2])))
        res = []
        for o, n, mul in zip(outs, ns, (1, 8, 1)):
            a = np.ctypeslib.as_array(o, shape=(max(1, n.value * mul),))[:n.value * mul].copy()
            self.L.nx_free_host(o)
            res.append(a)
        return res[0], res[1].reshape(-1, 8), res[2]

    def fri_decompose(self, src4):
        g = DeviceColumns(self, 4, src4.log_size)
        lam = np.zeros(4, np.uint32)
        self._chk(self.L.nx_fri_decompose(self.ctx, src4.col_ptrs(), src4.log_size, g.col_ptrs(), lam.ctypes.data_as(C.c_void_p)))
        return g, lam

    # ---- QuotientOps ----
    def accumulate_quotients(self, cols, random_coeff, batches):
        """batches: list of (point8, [(col_idx, value4), ...]).  Returns a 4-column DeviceColumns."""
        out = DeviceColumns(self, 4, cols.log_size)
        pts = _u32([b[0] for b in batches]).reshape(-1)
        counts = _u32([len(b[1]) for b in batches])
        cidx = _u32([cv[0] for b in batches for cv in b[1]])
        vals = _u32([cv[1] for b in batches for cv in b[1]]).reshape(-1)
        a = _u32(random_coeff)
        self._chk(self.L.nx_accumulate_quotients(self.ctx, cols.log_size, cols.col_ptrs(), cols.n_cols, a.ctypes.data_as(C.c_void_p),
                                                 len(batches), pts.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                 cidx.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), out.col_ptrs()))
        return out

    def accumulate_quotients_partial(self, cols, log_size, random_coeff, batches, entry_local, include_line_terms, out=None):
        """nx_accumulate_quotients_partial, one rank's share of a column-sharded quotient: cols = the DeviceColumns this rank holds (None:
        it holds none), batches as for accumulate_quotients but over ALL entries, a local entry's col_idx counted in `cols`, any other's
        ignored; entry_local = one flag per flattened entry (None: all local).  Returns the 4-column partial sum (written into `out`)."""
        out = DeviceColumns(self, 4, log_size) if out is None else out
        pts = _u32([b[0] for b in batches]).reshape(-1)
        counts = _u32([len(b[1]) for b in batches])
        cidx = _u32([cv[0] for b in batches for cv in b[1]])
        vals = _u32([cv[1] for b in batches for cv in b[1]]).reshape(-1)
        a = _u32(random_coeff)
        loc = None if entry_local is None else np.ascontiguousarray(entry_local, dtype=np.uint8)
        self._chk(self.L.nx_accumulate_quotients_partial(self.ctx, log_size, cols.col_ptrs() if cols is not None else None,
                                                         cols.n_cols if cols is not None else 0, a.ctypes.data_as(C.c_void_p),
                                                         len(batches), pts.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                         cidx.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p),
                                                         loc.ctypes.data_as(C.c_void_p) if loc is not None else None, int(bool(include_line_terms)),
                                                         out.col_ptrs()))
        return out

    # ---- recorded AIR constraints ----
    def eval_constraint_program(self, program, column_ptrs, alpha_powers, denom_inv, log_size, log_eval, acc4):
        """Run an air_program.Program over every row of the evaluation domain and accumulate into acc4 (a 4-column
        DeviceColumns of log size log_eval).  column_ptrs: device addresses (ints) of the columns the program's LOADs index."""
        ins = _u32(program.instrs).reshape(-1)
        ptrs = (C.c_void_p * max(1, len(column_ptrs)))(*column_ptrs)
        ec = _u32(program.econsts).reshape(-1)
        pw = _u32(alpha_powers).reshape(-1)
        den = _u32(denom_inv)
        self._chk(self.L.nx_eval_constraint_program(self.ctx, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, ptrs, len(column_ptrs),
                                                    ec.ctypes.data_as(C.c_void_p), len(ec) // 4, pw.ctypes.data_as(C.c_void_p), len(pw) // 4,
                                                    den.ctypes.data_as(C.c_void_p), log_size, log_eval, acc4.col_ptrs()))
        return acc4

    def air_check(self, program, column_ptrs, log_size, max_failures=64, econsts=None):
        """nx_air_check: every constraint of an air_program.Program on every row of the trace domain.  column_ptrs: device addresses
        (ints; None for columns no constraint loads) of trace-domain evaluations.  Returns a CheckReport."""
        ins = _u32(program.instrs).reshape(-1)
        ptrs = (C.c_void_p * max(1, len(column_ptrs)))(*column_ptrs)
        ec = _u32(program.econsts if econsts is None else econsts).reshape(-1)
        out = (CheckFailureC * max(1, max_failures))()
        n = C.c_uint32(0)
        rc = self.L.nx_air_check(self.ctx, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, ptrs, len(column_ptrs),
                                 ec.ctypes.data_as(C.c_void_p) if len(ec) else None, len(ec) // 4, program.n_constraints, log_size, out, int(max_failures), C.byref(n))
        return _check_report(self, rc, out, n, max_failures)

    def prover_session(self, cfg, max_log_size):
        return ProverSession(self, cfg, max_log_size)

    def compile_air(self, program, n_cols, select=None):
        """nx_air_compile(_subset): the recorded program as a run-time-compiled gfx950 kernel (same semantics as the interpreter)."""
        return AirKernel(self, program, n_cols, select)

    # ---- logup interaction trace ----
    @staticmethod
    def _ptr4(cols4):
        return cols4.col_ptrs() if cols4 is not None else None

    def logup_combine(self, tuple_cols, alpha_powers, z):
        """Relation::combine over device columns: sum_i alpha_powers[i] * tuple_i - z -> a secure (4-column) DeviceColumns."""
        out = DeviceColumns(self, 4, tuple_cols.log_size)
        ap, zz = _u32(alpha_powers).reshape(-1), _u32(z)
        self._chk(self.L.nx_logup_combine(self.ctx, tuple_cols.col_ptrs(), tuple_cols.n_cols, ap.ctypes.data_as(C.c_void_p), zz.ctypes.data_as(C.c_void_p),
                                          tuple_cols.log_size, out.col_ptrs()))
        return out

    def logup_finalize_col(self, den_a, scale_a=(1, 0, 0, 0), mult_a=None, den_b=None, scale_b=(1, 0, 0, 0), mult_b=None, prev=None, out=None):
        """LogupColGenerator::write_frac + finalize_col (one fraction, or two merged as prover2 does).  mult_*: a 1-column
        DeviceColumns (numerator = scale * mult) or None (numerator = scale)."""
        out = out or DeviceColumns(self, 4, den_a.log_size)
        sa, sb = _u32(scale_a), _u32(scale_b)
        self._chk(self.L.nx_logup_finalize_col(self.ctx, den_a.log_size, mult_a.ptr if mult_a is not None else None, sa.ctypes.data_as(C.c_void_p),
                                               den_a.col_ptrs(), mult_b.ptr if mult_b is not None else None, sb.ctypes.data_as(C.c_void_p),
                                               self._ptr4(den_b), self._ptr4(prev), out.col_ptrs()))
        return out

    def logup_col(self, frac_a, frac_b=None, prev=None, out=None):
        """Fused combine + write_frac + finalize_col (nx_logup_col).  A fraction is a dict: tuple (DeviceColumns), alphas
        (n x 4), z (4), optional mult (1-column DeviceColumns), optional scale (4, default 1)."""
        keep = []

        def mk(f):
            t = f["tuple"]
            ptrs = t.col_ptrs(); ap = _u32(f["alphas"]).reshape(-1); z = _u32(f["z"]); sc = _u32(f.get("scale", (1, 0, 0, 0)))
            keep.extend([ptrs, ap, z, sc])
            m = f.get("mult")
            return LogupFrac(C.cast(ptrs, C.c_void_p), t.n_cols, ap.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p),
                             m.ptr if m is not None else None, sc.ctypes.data_as(C.c_void_p))
        fa = mk(frac_a)
        fb = mk(frac_b) if frac_b is not None else None
        out = out or DeviceColumns(self, 4, frac_a["tuple"].log_size)
        self._chk(self.L.nx_logup_col(self.ctx, frac_a["tuple"].log_size, C.byref(fa), C.byref(fb) if fb is not None else None, self._ptr4(prev), out.col_ptrs()))
        return out

    def logup_cols(self, fracs):
        """All the logup columns of a component in one launch (nx_logup_cols): column j = sum of the first j + 1 fractions of the
        row.  fracs: dicts as for logup_col.  Returns one 4-column DeviceColumns per fraction."""
        keep, arr = [], (LogupFrac * len(fracs))()
        for i, f in enumerate(fracs):
            t = f["tuple"]
            ptrs = t.col_ptrs(); ap = _u32(f["alphas"]).reshape(-1); z = _u32(f["z"]); sc = _u32(f.get("scale", (1, 0, 0, 0)))
            keep.extend([ptrs, ap, z, sc])
            m = f.get("mult")
            arr[i] = LogupFrac(C.cast(ptrs, C.c_void_p), t.n_cols, ap.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p),
                               m.ptr if m is not None else None, sc.ctypes.data_as(C.c_void_p))
        log = fracs[0]["tuple"].log_size
        outs = [DeviceColumns(self, 4, log) for _ in fracs]
        ptrs = (C.c_void_p * (4 * len(fracs)))(*[o.ptr.value + k * (4 << log) for o in outs for k in range(4)])
        self._chk(self.L.nx_logup_cols(self.ctx, log, arr, len(fracs), ptrs))
        return outs

    def logup_cols_batched(self, fracs, batching=None, n_cols=None):
        """finalize_logup_batched on the trace side (nx_logup_cols_batched): fraction i belongs to batch batching[i] (None: in pairs,
        i // 2), column j = the sum of the fractions of batches <= j.  Returns one 4-column DeviceColumns per logup column."""
        keep, arr = [], (LogupFrac * len(fracs))()
        for i, f in enumerate(fracs):
            t = f["tuple"]
            ptrs = t.col_ptrs(); ap = _u32(f["alphas"]).reshape(-1); z = _u32(f["z"]); sc = _u32(f.get("scale", (1, 0, 0, 0)))
            keep.extend([ptrs, ap, z, sc])
            m = f.get("mult")
            arr[i] = LogupFrac(C.cast(ptrs, C.c_void_p), t.n_cols, ap.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p),
                               m.ptr if m is not None else None, sc.ctypes.data_as(C.c_void_p))
        log = fracs[0]["tuple"].log_size
        if n_cols is None:
            n_cols = (len(fracs) + 1) // 2 if batching is None else max(batching) + 1
        outs = [DeviceColumns(self, 4, log) for _ in range(n_cols)]
        ptrs = (C.c_void_p * (4 * n_cols))(*[o.ptr.value + k * (4 << log) for o in outs for k in range(4)])
        b = None if batching is None else _u32(batching)
        self._chk(self.L.nx_logup_cols_batched(self.ctx, log, arr, len(fracs), b.ctypes.data_as(C.c_void_p) if b is not None else None, n_cols, ptrs))
        return outs

    def logup_program(self, program, column_ptrs, log_size, n_logup_cols=None, econsts=None, out_ptrs=None):
        """The interaction trace of a component from the relation entries its recorded AIR declares (nx_logup_program): program =
        ProgramBuilder.build_logup(); column_ptrs: one device pointer per component column (None where the program loads nothing).
        Returns one 4-column DeviceColumns per logup column (follow with logup_finalize_last on the last one) — or, with out_ptrs
        (4 device pointers per logup column, e.g. a session's own interaction-tree columns from tree_begin), writes there and returns
        out_ptrs: nothing is copied afterwards (rust/nexus-hip/src/simd_host.rs interaction_tree_on_device)."""
        n_logup_cols = program.n_logup_cols if n_logup_cols is None else n_logup_cols
        ins = _u32(program.instrs).reshape(-1)
        ec = _u32(program.econsts if econsts is None else econsts).reshape(-1)
        ptrs = (C.c_void_p * max(1, len(column_ptrs)))(*column_ptrs)
        if out_ptrs is None:
            outs = [DeviceColumns(self, 4, log_size) for _ in range(n_logup_cols)]
            flat = [o.ptr.value + k * (4 << log_size) for o in outs for k in range(4)]
        else:
            outs, flat = out_ptrs, [int(x) for x in out_ptrs]
            if len(flat) != 4 * n_logup_cols:
                raise NexusHipError(f"logup_program: {len(flat)} output columns for {n_logup_cols} logup columns")
        optr = (C.c_void_p * max(1, 4 * n_logup_cols))(*flat)
        self._chk(self.L.nx_logup_program(self.ctx, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, ptrs, len(column_ptrs),
                                          ec.ctypes.data_as(C.c_void_p) if len(ec) else None, len(ec) // 4, log_size, n_logup_cols, optr, None))
        return outs

    def trace_program(self, program, cols, log_size):
        """nx_trace_program: derived trace columns filled on the device.  program = ProgramBuilder.build_trace_program(); cols: one
        device address (int) per column of the table the program's LOADs and stores index — trace-domain evaluations of 2^log_size
        words, e.g. what ProverSession.tree_begin handed out (None where the program touches nothing).  Stream-ordered."""
        ins = _u32(program.instrs).reshape(-1)
        ptrs = (C.c_void_p * max(1, len(cols)))(*[int(c) if c else None for c in cols])
        self._chk(self.L.nx_trace_program(self.ctx, ins.ctypes.data_as(C.c_void_p), len(ins) // 4, program.n_regs, ptrs, len(cols), int(log_size), None))

    def logup_finalize_last(self, col4, log_size=None):
        """LogupTraceGenerator::finalize_last in place; returns the claimed sum (4 words).  col4: a 4-column DeviceColumns, or (with
        log_size) the 4 device pointers of the coordinate columns."""
        cs = np.zeros(4, np.uint32)
        if log_size is None:
            log_size, ptrs = col4.log_size, col4.col_ptrs()
        else:
            ptrs = (C.c_void_p * 4)(*[int(x) for x in col4])
        self._chk(self.L.nx_logup_finalize_last(self.ctx, log_size, ptrs, cs.ctypes.data_as(C.c_void_p)))
        return cs

    def logup_finalize_last_batch(self, cols4_list):
        """finalize_last for several secure columns of one size in one call; returns the claimed sums (n x 4)."""
        n = len(cols4_list)
        ptrs = (C.c_void_p * max(1, 4 * n))(*[c.ptr.value + q * (4 << c.log_size) for c in cols4_list for q in range(4)])
        cs = np.zeros((n, 4), np.uint32)
        self._chk(self.L.nx_logup_finalize_last_batch(self.ctx, cols4_list[0].log_size if n else 0, ptrs, n, cs.ctypes.data_as(C.c_void_p)))
        return cs

    def logup_multiplicities(self, uses, table_ptrs, log_table, key_bits, out_ptr, want_rc=False):
        """The table side of a lookup (nx_logup_multiplicities): out_ptr[pos] = how often (weighted, mod p) the key of table row pos
        occurs in `uses`.  uses: (value_ptrs, weight_ptr or None, log_size) each, value_ptrs = one device pointer per key column in
        any row order; table_ptrs: the table's key columns (2^log_table words each); key_bits: bits per key column; out_ptr: device
        pointer of 2^log_table words, e.g. the table component's main column from ProverSession.tree_begin.  Returns (n_missing,
        first_use, first_pos) of the rows that are in no table row — (0, 0, 0) when the lookup is sound; raises as the neighbours do
        on every code but NX_ERR_PROTOCOL (rows missing: the counts of the others are still written).  want_rc: also the code."""
        kb = _u32(key_bits).reshape(-1)
        k = len(kb)
        if len(table_ptrs) != k:
            raise NexusHipError(f"logup_multiplicities: {len(table_ptrs)} table columns for {k} key columns")
        arr, keep = (LookupUse * max(1, len(uses)))(), []
        for i, (vals, weight, log_size) in enumerate(uses):
            if len(vals) != k:
                raise NexusHipError(f"logup_multiplicities: use {i} has {len(vals)} value columns for {k} key columns")
            vp = (C.c_void_p * k)(*[int(v) for v in vals])
            keep.append(vp)
            arr[i] = LookupUse(C.cast(vp, C.c_void_p), int(weight) if weight is not None else None, int(log_size))
        tp = (C.c_void_p * k)(*[int(t) for t in table_ptrs])
        n, fu, fp = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        rc = self.L.nx_logup_multiplicities(self.ctx, arr, len(uses), k, kb.ctypes.data_as(C.c_void_p), tp, int(log_table), C.c_void_p(int(out_ptr)),
                                            C.byref(n), C.byref(fu), C.byref(fp))
        if rc not in (NX_OK, NX_ERR_PROTOCOL):
            self._chk(rc)
        res = (n.value, fu.value, fp.value)
        return (res, rc) if want_rc else res

    def logup_multiplicities_sparse(self, uses, table_ptrs, valid_ptr, log_table, key_bits, out_ptr, want_rc=False):
        """logup_multiplicities for a table that is a sparse subset of a key space of up to 32 bits (nx_logup_multiplicities_sparse):
        the boundary tables keyed by an address.  uses, table_ptrs, key_bits, out_ptr and the result are those of
        logup_multiplicities; valid_ptr: None (every row is a table row) or the device pointer of 2^log_table words, a row being a
        table row iff its word is nonzero.  out_ptr gets 0 on the other rows.  Temporaries follow the table's rows, not the key
        space."""
        kb = _u32(key_bits).reshape(-1)
        k = len(kb)
        if len(table_ptrs) != k:
            raise NexusHipError(f"logup_multiplicities_sparse: {len(table_ptrs)} table columns for {k} key columns")
        arr, keep = (LookupUse * max(1, len(uses)))(), []
        for i, (vals, weight, log_size) in enumerate(uses):
            if len(vals) != k:
                raise NexusHipError(f"logup_multiplicities_sparse: use {i} has {len(vals)} value columns for {k} key columns")
            vp = (C.c_void_p * k)(*[int(v) for v in vals])
            keep.append(vp)
            arr[i] = LookupUse(C.cast(vp, C.c_void_p), int(weight) if weight is not None else None, int(log_size))
        tp = (C.c_void_p * max(1, k))(*[int(t) for t in table_ptrs])
        n, fu, fp = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        rc = self.L.nx_logup_multiplicities_sparse(self.ctx, arr, len(uses), k, kb.ctypes.data_as(C.c_void_p), tp,
                                                   C.c_void_p(int(valid_ptr)) if valid_ptr is not None else None, int(log_table),
                                                   C.c_void_p(int(out_ptr)) if out_ptr is not None else None, C.byref(n), C.byref(fu), C.byref(fp))
        if rc not in (NX_OK, NX_ERR_PROTOCOL):
            self._chk(rc)
        res = (n.value, fu.value, fp.value)
        return (res, rc) if want_rc else res

    def trace_prev_access(self, streams, key_bits, n_payload, init=None, summary=None, want_rc=False):
        """The memory-checking columns (nx_trace_prev_access): for every access, what the previous access to the same key left behind.
        streams: dicts in time order within a row — key: one device pointer per key column; log_size; optional flag (pointer, None:
        every row accesses), payload (n_payload pointers, None entries read as 0), prev (n_payload output pointers or None entries;
        absent: no output), ordinal (output pointer), epoch (default 0), linear (default False: bit-reversed circle-domain order).
        key_bits: bits per key column; init: n_payload words an untouched key reads (default 0); summary: (cap, key_ptr, count_ptr,
        last_ptrs) — one entry per distinct key in ascending order, the first min(cap, n_keys) written.  Returns the number of distinct
        keys; raises as the neighbours do, also on NX_ERR_PROTOCOL (an accessing row with a key entry outside its bits) unless
        want_rc: then (n_keys or None, code)."""
        kb = _u32(key_bits).reshape(-1)
        k, n_payload = len(kb), int(n_payload)

        def table(ptrs, n, what, i):
            if ptrs is None:
                return None
            if len(ptrs) != n:
                raise NexusHipError(f"trace_prev_access: stream {i} has {len(ptrs)} {what} columns, {n} expected")
            t = (C.c_void_p * max(1, n))(*[int(x) if x else None for x in ptrs])
            keep.append(t)
            return C.cast(t, C.c_void_p)

        arr, keep = (AccessStream * max(1, len(streams)))(), []
        for i, s in enumerate(streams):
            arr[i] = AccessStream(table(s["key"], k, "key", i), int(s["flag"]) if s.get("flag") else None, table(s.get("payload"), n_payload, "payload", i),
                                  table(s.get("prev"), n_payload, "prev", i), int(s["ordinal"]) if s.get("ordinal") else None, int(s["log_size"]),
                                  int(s.get("epoch", 0)), int(bool(s.get("linear", False))))
        iv = None
        if init is not None:
            iv = _u32(init).reshape(-1)
            if len(iv) != n_payload:
                raise NexusHipError(f"trace_prev_access: {len(iv)} init words for {n_payload} payload columns")
        sm = None
        if summary is not None:
            cap, key_ptr, count_ptr, last_ptrs = summary
            sm = AccessSummary(int(cap), int(key_ptr) if key_ptr else None, int(count_ptr) if count_ptr else None, table(last_ptrs, n_payload, "summary last", "-"))
        n = C.c_uint64(0)
        rc = self.L.nx_trace_prev_access(self.ctx, arr, len(streams), k, kb.ctypes.data_as(C.c_void_p), n_payload, iv.ctypes.data_as(C.c_void_p) if iv is not None else None,
                                         C.byref(sm) if sm is not None else None, C.byref(n))
        if want_rc and rc in (NX_OK, NX_ERR_PROTOCOL):
            return (n.value if rc == NX_OK else None), rc
        self._chk(rc)
        return n.value

    def trace_access_chain(self, streams, key_bits, n_payload, init=None, summary=None, want_rc=False):
        """nx_trace_access_chain: trace_prev_access for accesses that leave behind what depends on what they found, and for block
        records.  streams: the dicts of trace_prev_access, and further — rule: n_payload words of CHAIN_GIVEN / CHAIN_ADD
        (| CHAIN_BYTES), absent: all GIVEN; delta: n_payload words added by the ADD columns, absent: all 1; row: device pointer of
        n_records strictly ascending natural rows, which makes the stream a BLOCK stream of n_records records of `span` accesses to
        key + i (key and flag then hold one word per record, payload / prev / ordinal one word per access, record-major; a
        CHAIN_BYTES payload one byte per access).  Returns the number of distinct keys; raises as the neighbours do, also on
        NX_ERR_PROTOCOL (a key outside its bits, rows that do not ascend) unless want_rc: then (n_keys or None, code)."""
        kb = _u32(key_bits).reshape(-1)
        k, n_payload = len(kb), int(n_payload)

        def table(ptrs, n, what, i):
            if ptrs is None:
                return None
            if len(ptrs) != n:
                raise NexusHipError(f"trace_access_chain: stream {i} has {len(ptrs)} {what} columns, {n} expected")
            t = (C.c_void_p * max(1, n))(*[int(x) if x else None for x in ptrs])
            keep.append(t)
            return C.cast(t, C.c_void_p)

        def words(vals, what, i):
            if vals is None:
                return None
            if len(vals) != n_payload:
                raise NexusHipError(f"trace_access_chain: stream {i} has {len(vals)} {what} words, {n_payload} expected")
            t = (C.c_uint32 * max(1, n_payload))(*[int(x) & 0xFFFFFFFF for x in vals])
            keep.append(t)
            return C.cast(t, C.c_void_p)

        arr, keep = (ChainStream * max(1, len(streams)))(), []
        for i, s in enumerate(streams):
            arr[i] = ChainStream(table(s["key"], k, "key", i), int(s["flag"]) if s.get("flag") else None, int(s["row"]) if s.get("row") else None,
                                 table(s.get("payload"), n_payload, "payload", i), words(s.get("rule"), "rule", i), words(s.get("delta"), "delta", i),
                                 table(s.get("prev"), n_payload, "prev", i), int(s["ordinal"]) if s.get("ordinal") else None, int(s.get("log_size", 0)),
                                 int(s.get("n_records", 0)), int(s.get("span", 0)), int(s.get("epoch", 0)), int(bool(s.get("linear", False))))
        iv = None
        if init is not None:
            iv = _u32(init).reshape(-1)
            if len(iv) != n_payload:
                raise NexusHipError(f"trace_access_chain: {len(iv)} init words for {n_payload} payload columns")
        sm = None
        if summary is not None:
            cap, key_ptr, count_ptr, last_ptrs = summary
            sm = AccessSummary(int(cap), int(key_ptr) if key_ptr else None, int(count_ptr) if count_ptr else None, table(last_ptrs, n_payload, "summary last", "-"))
        n = C.c_uint64(0)
        rc = self.L.nx_trace_access_chain(self.ctx, arr, len(streams), k, kb.ctypes.data_as(C.c_void_p), n_payload, iv.ctypes.data_as(C.c_void_p) if iv is not None else None,
                                          C.byref(sm) if sm is not None else None, C.byref(n))
        if want_rc and rc in (NX_OK, NX_ERR_PROTOCOL):
            return (n.value if rc == NX_OK else None), rc
        self._chk(rc)
        return n.value

    def trace_keccak_round(self, states_ptr, n_instances, first_round, log_rounds, log_size, main_ptrs, pre_ptrs=None, states_out_ptr=None):
        """nx_trace_keccak_round: the KeccakRound component's trace filled on the device.  states_ptr: device address of n_instances x 25
        64-bit lanes (index x + 5 y; None when n_instances is 0); natural row instance * 2^log_rounds + i holds round first_round + i.
        main_ptrs: KECCAK_ROUND_MAIN_COLS device addresses of 2^log_size words, e.g. what ProverSession.tree_begin handed out; pre_ptrs:
        None or KECCAK_ROUND_PRE_COLS addresses (round-constant bytes, is_last); states_out_ptr: None or n_instances x 25 lanes, the
        state after the component's last round.  Stream-ordered."""
        if len(main_ptrs) != KECCAK_ROUND_MAIN_COLS:
            raise NexusHipError(f"trace_keccak_round: {len(main_ptrs)} main columns, {KECCAK_ROUND_MAIN_COLS} expected")
        if pre_ptrs is not None and len(pre_ptrs) != KECCAK_ROUND_PRE_COLS:
            raise NexusHipError(f"trace_keccak_round: {len(pre_ptrs)} preprocessed columns, {KECCAK_ROUND_PRE_COLS} expected")
        mp = (C.c_void_p * KECCAK_ROUND_MAIN_COLS)(*[int(x) if x else None for x in main_ptrs])
        pp = (C.c_void_p * KECCAK_ROUND_PRE_COLS)(*[int(x) if x else None for x in pre_ptrs]) if pre_ptrs is not None else None
        self._chk(self.L.nx_trace_keccak_round(self.ctx, C.c_void_p(int(states_ptr)) if states_ptr else None, C.c_uint32(int(n_instances)), C.c_uint32(int(first_round)),
                                               C.c_uint32(int(log_rounds)), C.c_uint32(int(log_size)), mp, pp, C.c_void_p(int(states_out_ptr)) if states_out_ptr else None))

    def trace_keccak_memory_check(self, states_ptr, addresses_ptr, timestamps_ptr, n_instances, log_size, main_ptrs, pre_ptrs=None, states_out_ptr=None):
        """nx_trace_keccak_memory_check: the PermutationMemoryCheck component's trace filled on the device.  states_ptr: device address of
        n_instances x 25 64-bit lanes, addresses_ptr: n_instances words, timestamps_ptr: n_instances x 200 words, 16-byte aligned (each
        None when n_instances is 0); natural row r is instance r.  main_ptrs: KECCAK_MEMCHECK_MAIN_COLS device addresses of 2^log_size
        words, e.g. what ProverSession.tree_begin handed out; pre_ptrs: None or the one is_last column; states_out_ptr: None or
        n_instances x 25 lanes, keccak-f[1600] of the inputs.  addr + i and ts + 1 are taken modulo 2^32.  Stream-ordered."""
        if len(main_ptrs) != KECCAK_MEMCHECK_MAIN_COLS:
            raise NexusHipError(f"trace_keccak_memory_check: {len(main_ptrs)} main columns, {KECCAK_MEMCHECK_MAIN_COLS} expected")
        if pre_ptrs is not None and len(pre_ptrs) != KECCAK_MEMCHECK_PRE_COLS:
            raise NexusHipError(f"trace_keccak_memory_check: {len(pre_ptrs)} preprocessed columns, {KECCAK_MEMCHECK_PRE_COLS} expected")
        mp = (C.c_void_p * KECCAK_MEMCHECK_MAIN_COLS)(*[int(x) if x else None for x in main_ptrs])
        pp = (C.c_void_p * KECCAK_MEMCHECK_PRE_COLS)(*[int(x) if x else None for x in pre_ptrs]) if pre_ptrs is not None else None
        dev = lambda p: C.c_void_p(int(p)) if p else None
        self._chk(self.L.nx_trace_keccak_memory_check(self.ctx, dev(states_ptr), dev(addresses_ptr), dev(timestamps_ptr), C.c_uint32(int(n_instances)),
                                                      C.c_uint32(int(log_size)), mp, pp, dev(states_out_ptr)))

    def trace_partition(self, class_ptr, n_steps, n_classes, want_rc=False):
        """nx_trace_partition_create: the steps of an execution split by class.  class_ptr: device address of n_steps words, the
        component of every step (0 .. n_classes - 1, or PART_NONE: in no component).  Returns (counts, handle): the steps of every class
        as a uint32 array, and a TracePartition whose fill(...) makes the components' columns and whose destroy() releases the order
        (n_steps words of device memory).  Blocking.  Raises as the neighbours do, also on NX_ERR_PROTOCOL (a class word outside the
        classes; the message names the smallest such step) unless want_rc: then (counts or None, handle or None, code)."""
        counts = np.zeros(max(1, int(n_classes)), np.uint32)
        h = C.c_void_p()
        rc = self.L.nx_trace_partition_create(self.ctx, C.c_void_p(int(class_ptr)) if class_ptr else None, C.c_uint32(int(n_steps)), C.c_uint32(int(n_classes)),
                                              counts.ctypes.data_as(C.c_void_p), C.byref(h))
        if want_rc and rc in (NX_OK, NX_ERR_PROTOCOL, NX_ERR_ARG):
            ok = rc == NX_OK
            return (counts[:int(n_classes)] if ok else None), (TracePartition(self, h, counts[:int(n_classes)], int(n_steps)) if ok else None), rc
        self._chk(rc)
        counts = counts[:int(n_classes)]
        return counts, TracePartition(self, h, counts, int(n_steps))

    # ---- FriOps ----
    def fold_circle_into_line(self, tw, dst4, src4, alpha):
        a = _u32(alpha)
        self._chk(self.L.nx_fold_circle_into_line(self.ctx, tw.h, dst4.col_ptrs(), src4.col_ptrs(), src4.log_size, a.ctypes.data_as(C.c_void_p)))
        return dst4

    def fold_line(self, tw, src4, alpha, n_doublings=0):
        out = DeviceColumns(self, 4, src4.log_size - 1)
        a = _u32(alpha)
        self._chk(self.L.nx_fold_line(self.ctx, tw.h, src4.col_ptrs(), src4.log_size, n_doublings, a.ctypes.data_as(C.c_void_p), out.col_ptrs()))
        return out

    # ---- GrindOps ----
    def grind(self, digest_words, pow_bits):
        d = _u32(digest_words)
        nonce = C.c_uint64()
        self._chk(self.L.nx_grind(self.ctx, d.ctypes.data_as(C.c_void_p), pow_bits, C.byref(nonce)))
        return nonce.value

    # ---- synthetic machine ----
    @staticmethod
    def _comps(comps):
        return (ComponentSpec * len(comps))(*[ComponentSpec(*[int(x) for x in c]) for c in comps])   # 4-, 5- or 6-tuples (bound and logup_mode default to 0)

    def synth_fill_tree(self, comps, tree, seed, inter_seed=0):
        sets = []
        ptrs = []
        for (ls, a, b, c) in [tuple(x)[:4] for x in comps]:
            n = [a, b, c][tree]
            s = DeviceColumns(self, n, ls)
            sets.append(s)
            ptrs += [s.ptr.value + i * (4 << ls) for i in range(n)]
        arr = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        self._chk(self.L.nx_synth_fill_tree(self.ctx, self._comps(comps), len(comps), tree, C.c_uint64(seed), C.c_uint64(inter_seed), arr))
        return sets

    def prove(self, comps, cfg=None, seed=1, ad=b"", want_stats=False):
        """nexus_vm_prover::prove analogue for the synthetic machine (reference prover/src/lib.rs:26-31)."""
        cfg = cfg or default_config()
        words, n = C.POINTER(C.c_uint32)(), C.c_size_t(0)
        stats = ProveStats()
        adb = (C.c_uint8 * max(1, len(ad)))(*ad)
        self._chk(self.L.nx_prove_synth(self.ctx, self._comps(comps), len(comps), C.byref(cfg), C.c_uint64(seed), adb, C.c_size_t(len(ad)),
                                        C.byref(words), C.byref(n), C.byref(stats) if want_stats else None))
        out = np.ctypeslib.as_array(words, shape=(n.value,)).copy()
        self.L.nx_free_host(words)
        return (out, stats.as_dict()) if want_stats else out

    def prove_machine(self, comps, cfg=None, seed=1, ad=b"", want_stats=False, comm=None):
        """nexus_vm_prover::prove analogue with a REAL logup interaction trace and a recorded AIR (nx_prove_machine); comps:
        (log_size, n_pre, n_main, 4 x logup columns).  comm: an NxComm for ONE proof on several GPUs (every rank calls this)."""
        cfg = cfg or default_config()
        words, n = C.POINTER(C.c_uint32)(), C.c_size_t(0)
        stats = ProveStats()
        adb = (C.c_uint8 * max(1, len(ad)))(*ad)
        self._chk(self.L.nx_prove_machine(self.ctx, self._comps(comps), len(comps), C.byref(cfg), C.c_uint64(seed), adb, C.c_size_t(len(ad)),
                                          C.byref(comm) if comm is not None else None, C.byref(words), C.byref(n), C.byref(stats) if want_stats else None))
        out = np.ctypeslib.as_array(words, shape=(n.value,)).copy()
        self.L.nx_free_host(words)
        return (out, stats.as_dict()) if want_stats else out

    def prove_machine_host(self, comps, cfg, pre_cols, main_cols, ad=b"", coset_order=False, want_stats=False):
        """nx_prove_machine_host: the machine's preprocessed / main traces from HOST memory (lists of contiguous uint32 arrays, component
        after component), uploaded under the commits' own transforms.  Same proof as prove_machine for the same trace."""
        return self._prove_machine_host(comps, cfg, [_u32(c) for c in pre_cols], None, [_u32(c) for c in main_cols], None, ad, coset_order, want_stats)

    def prove_machine_host_narrow(self, comps, cfg, pre_cols, main_cols, ad=b"", coset_order=False, want_stats=False, pre_as=None, main_as=None):
        """nx_prove_machine_host_narrow: prove_machine_host with host columns of uint8 / uint16 / uint32 arrays (the kind follows the
        dtype; pre_as / main_as declare uint32 columns to hold byte or half-word values, as as_kind of upload_columns_narrow).  Same proof
        as prove_machine_host for the same values; a value that does not fit its declared width raises NexusHipError."""
        pre, pk = _narrow_columns(pre_cols, pre_as)
        main, mk = _narrow_columns(main_cols, main_as)
        return self._prove_machine_host(comps, cfg, pre, pk, main, mk, ad, coset_order, want_stats)

    def _prove_machine_host(self, comps, cfg, pre, pre_kinds, main, main_kinds, ad, coset_order, want_stats):
        """prove_machine_host (kinds None: nx_prove_machine_host) and prove_machine_host_narrow (nx_prove_machine_host_narrow)."""
        fn = self.L.nx_prove_machine_host if pre_kinds is None else self.L.nx_prove_machine_host_narrow
        cfg = cfg or default_config()
        words, n = C.POINTER(C.c_uint32)(), C.c_size_t(0)
        stats = ProveStats()
        adb = (C.c_uint8 * max(1, len(ad)))(*ad)
        self._chk(fn(self.ctx, self._comps(comps), len(comps), C.byref(cfg), *_host_columns(pre, pre_kinds), *_host_columns(main, main_kinds),
                     int(bool(coset_order)), adb, C.c_size_t(len(ad)), C.byref(words), C.byref(n), C.byref(stats) if want_stats else None))
        out = np.ctypeslib.as_array(words, shape=(n.value,)).copy()
        self.L.nx_free_host(words)
        return (out, stats.as_dict()) if want_stats else out

    def machine_claimed_sums(self):
        """`Proof.claimed_sum` of the last prove_machine on this context (reference machine.rs:93-98): (n_components, 4) uint32."""
        n = C.c_uint32(0)
        self._chk(self.L.nx_machine_claimed_sums(self.ctx, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), np.uint32)
        if n.value:
            self._chk(self.L.nx_machine_claimed_sums(self.ctx, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def prove_sharded(self, comps, comm, cfg=None, seed=1, ad=b"", want_stats=False):
        """One proof, columns sharded over the ranks of `comm` (an NxComm from make_comm); every rank calls this with the
        same arguments and gets the same proof, bit-identical to `prove` on one GPU (nx_prove_synth_sharded)."""
        cfg = cfg or default_config()
        words, n = C.POINTER(C.c_uint32)(), C.c_size_t(0)
        stats = ProveStats()
        adb = (C.c_uint8 * max(1, len(ad)))(*ad)
        self._chk(self.L.nx_prove_synth_sharded(self.ctx, self._comps(comps), len(comps), C.byref(cfg), C.c_uint64(seed), adb, C.c_size_t(len(ad)),
                                                C.byref(comm), C.byref(words), C.byref(n), C.byref(stats) if want_stats else None))
        out = np.ctypeslib.as_array(words, shape=(n.value,)).copy()
        self.L.nx_free_host(words)
        return (out, stats.as_dict()) if want_stats else out
