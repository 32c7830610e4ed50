"""GPU parity of the Blake2s leaf hashing at every shape at which the column loop takes another path (-m gpu).

The leaf kernels stream a row's columns 16 at a time (one 64-byte block) through two register sets that take turns, the loop
unrolled by two, with the last block (full or zero-padded) and an odd block left over handled outside it.  So the column counts
cover one padded block (1, 15), exact blocks (16, 32, 48), a padded block behind full ones (17, 31, 33), odd and even numbers of
blocks, and the headline prove's 347; the row counts a launch below one workgroup's worth per CU (2^8), about one resident
generation (2^13) and several (2^16).  Both forms of a column set are hashed: base + stride (the columns of one slab, in order) and a
pointer table (here: the same columns stored in reverse order).

Reference, hash mode 0: hashlib.blake2s over each row's little-endian words.  Hash mode 1 (raw compression chain on a zero state):
the CPU oracle's commit, as in test_gpu_parity.py::test_merkle_commit_matches_oracle.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch  # noqa: F401  (before libnexus_hip.so: see test_gpu_parity.py)

import oracle_lib as O

pytestmark = pytest.mark.gpu
P = O.P
COL_COUNTS = (1, 15, 16, 17, 31, 32, 33, 48, 347)
ROW_LOGS = (8, 13, 16)


@pytest.fixture(scope="module")
def be():
    import nexus_zkvm_amd as nz
    b = nz.HipBackend(0)
    yield b
    b.set_hash_mode(0)
    b.close()


@pytest.fixture(scope="module")
def values():
    """347 columns of 2^16 rows, generated once; every case hashes a corner [:n_cols, :n_rows] of it."""
    v = np.random.default_rng(20260).integers(0, P, (347, 1 << 16), dtype=np.uint32)
    v[:, :4] = np.array([0, 1, P - 1, 0x55555555 % P], np.uint32)      # boundary words in the first rows of every column
    v.setflags(write=False)
    return v


_ref_cache = {}


def ref_leaves(oracle, values, mode, n_cols, log):
    """The 2^log leaf digests (n x 8 words) of the first n_cols columns; computed once per shape."""
    key = (mode, n_cols, log)
    if key not in _ref_cache:
        sub = np.ascontiguousarray(values[:n_cols, :1 << log])
        if mode == 0:
            rows = np.ascontiguousarray(sub.T).astype("<u4")
            out = np.frombuffer(b"".join(hashlib.blake2s(r.tobytes()).digest() for r in rows), dtype="<u4").astype(np.uint32)
        else:
            _, layers = oracle.merkle_commit(list(sub), mode, want_layers=True)
            out = layers[:8 << log].copy()                                 # the oracle stores the leaf layer first
        _ref_cache[key] = out.reshape(-1, 8)
    return _ref_cache[key]


class Cols:
    """n_cols columns of 2^log rows on the device, as base + stride ("stride") or behind a pointer table ("table": the columns are
    stored in reverse order, so their addresses descend and no stride describes them)."""

    def __init__(self, be, vals, form):
        self.n_cols, n = vals.shape
        self.log = int(np.log2(n))
        self.slab = be.columns(self.n_cols, self.log)
        self.slab.upload(vals[::-1] if form == "table" else vals)
        stride = 4 << self.log
        order = range(self.n_cols - 1, -1, -1) if form == "table" else range(self.n_cols)
        self.addrs = [self.slab.ptr.value + k * stride for k in order]

    def ptrs(self, lo=0, hi=None):
        a = self.addrs[lo:hi]
        return (C.c_void_p * len(a))(*a), len(a)


def leaf_chain(be, cols, lo, hi, total, state, first):
    arr, n = cols.ptrs(lo, hi)
    be._chk(be.L.nx_merkle_leaf_chain(be.ctx, arr, n, cols.log, lo, total, None if first else C.c_void_p(state.ptr.value), C.c_void_p(state.ptr.value),
                                      C.c_uint64(0), C.c_uint64(1 << cols.log)))


def commit_leaves(be, nz, cols):
    arr, n = cols.ptrs()
    logs = np.full(n, cols.log, np.uint32)
    h = C.c_void_p()
    be._chk(be.L.nx_merkle_commit(be.ctx, arr, logs.ctypes.data_as(C.c_void_p), n, C.byref(h)))
    return nz.MerkleTree(be, h).layer(cols.log)


def forms(n_cols):
    return ("stride", "table") if n_cols > 1 else ("stride",)      # a single column has no second form


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n_cols", COL_COUNTS)
def test_leaf_digests(be, oracle, values, mode, n_cols):
    import nexus_zkvm_amd as nz
    be.set_hash_mode(mode)
    for log in ROW_LOGS:
        ref = ref_leaves(oracle, values, mode, n_cols, log)
        for form in forms(n_cols):
            cols = Cols(be, values[:n_cols, :1 << log], form)
            state = be.columns(8, log)
            leaf_chain(be, cols, 0, n_cols, n_cols, state, True)
            be.sync()
            assert np.array_equal(state.to_cpu().reshape(-1, 8), ref), ("leaf_chain", mode, n_cols, log, form)
            assert np.array_equal(commit_leaves(be, nz, cols), ref), ("commit", mode, n_cols, log, form)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("split", [16, 32, 336])
def test_chained_shards(be, oracle, values, mode, split):
    """347 columns fed in two calls, the chaining state carried from the first to the second through device memory."""
    be.set_hash_mode(mode)
    for log in ROW_LOGS:
        ref = ref_leaves(oracle, values, mode, 347, log)
        for form in ("stride", "table"):
            cols = Cols(be, values[:, :1 << log], form)
            state = be.columns(8, log)
            leaf_chain(be, cols, 0, split, 347, state, True)
            leaf_chain(be, cols, split, 347, 347, state, False)
            be.sync()
            assert np.array_equal(state.to_cpu().reshape(-1, 8), ref), (mode, split, log, form)


@pytest.mark.parametrize("form", ["stride", "table"])
@pytest.mark.parametrize("mode", [0, 1])
def test_injected_inner_columns(be, oracle, values, mode, form):
    """A tree whose inner levels take columns of their own: 2^12 rows (33 columns: full blocks and a padded one behind the two child
    digests), 2^11 rows (16: one exact block) and 2^10 rows (a single column), above 17 leaf columns of 2^13 rows.  In the table form the
    columns of every level are stored in reverse order, so each level's set reaches its kernel as a pointer table."""
    import nexus_zkvm_amd as nz
    be.set_hash_mode(mode)
    shape = [(13, 17), (12, 33), (11, 16), (10, 1)]
    host, sets, c0 = [], [], 0
    for log, n in shape:
        host += [np.ascontiguousarray(values[c0 + k, :1 << log]) for k in range(n)]
        sets.append(Cols(be, values[c0:c0 + n, :1 << log], form))
        c0 += n
    root, layers = oracle.merkle_commit(host, mode, want_layers=True)
    addrs = [a for cs in sets for a in cs.addrs]
    logs = np.array([cs.log for cs in sets for _ in cs.addrs], np.uint32)
    h = C.c_void_p()
    be._chk(be.L.nx_merkle_commit(be.ctx, (C.c_void_p * len(addrs))(*addrs), logs.ctypes.data_as(C.c_void_p), len(addrs), C.byref(h)))
    tree = nz.MerkleTree(be, h)
    assert np.array_equal(tree.root(), root)
    off = 0
    for k in range(13, -1, -1):
        assert np.array_equal(tree.layer(k).reshape(-1), layers[off:off + (8 << k)]), (mode, form, k)
        off += 8 << k
