"""Column placement: where the columns of a call lie in device memory.

Every other GPU test allocates its columns with nx_alloc, 256-byte aligned and padded, so a store one word past a column, the word
fallbacks the host selects for columns that are not 16-byte aligned, and a wide access on a caller pointer never show.  Here a call's
columns are laid out by hand in ONE slab (Arena): every column at a chosen word offset modulo 4, at least GUARD words of FILL before and
after it, every output FILL before the call.  After the call the downloaded slab is checked: guards intact, inputs byte-identical,
outputs bit-equal to the oracle.  FILL >= p, so a word read out of a guard into the arithmetic also breaks the comparison.

This module imports nothing from the GPU: the layout, the classification table, the case list and the oracle side of every case are
plain numpy + the CPU oracle.  tests/test_placement_cpu.py pins them; tests/test_gpu_placement.py runs them on the device.

CLASSES (TABLE below, one row per public entry that reads or writes device columns; every row cites the access and the dispatch)
  S  word accesses only on caller pointers: the oracle's words at every shift.
  B  the host branches on the pointers' low bits between a 16-byte path and a word path: the oracle's words at every shift, at a size
     where the 16-byte path would otherwise run (Row.vector_from names it from the dispatch condition).
  W  an unconditional 16- or 8-byte access on a caller pointer: the entry refuses a misaligned pointer with NX_ERR_ARG before anything is
     launched (include/nexus_hip.h, "Alignment"); the test asserts the refusal and never launches the kernel on such a pointer.  Columns
     shorter than the access go through a word kernel and are accepted at every shift (Row.exempt_below)."""
import ctypes as C
from collections import namedtuple

import numpy as np

import oracle_lib as O

P = O.P
FILL = 0xDEADBEEF
GUARD = 64
SHIFTS = (0, 1, 2, 3)


# ------------------------------------------------------------------------------------------------------------------ the arena

class Col:
    def __init__(self, name, start, words, data):
        self.name, self.start, self.words, self.data = name, start, words, data

    @property
    def end(self):
        return self.start + self.words


class Arena:
    """A pure-numpy plan of one device slab (whose base is 16-byte aligned): add() places a column at `shift` words modulo 4 behind a
    guard of >= GUARD words; image() is the slab before the call; check() judges the slab after it."""

    def __init__(self):
        self.cols, self.end = {}, 0

    def add(self, name, data=None, words=None, shift=0):
        """data: the words uploaded (an input, or the start value of an in-place column); None: an output of `words` words, FILL."""
        assert name not in self.cols and shift in SHIFTS
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1).copy()
            words = data.size
        start = (self.end + GUARD + 3) // 4 * 4 + shift
        self.cols[name] = Col(name, start, int(words), data)
        self.end = start + int(words)
        return name

    @property
    def size(self):
        return (self.end + GUARD + 3) // 4 * 4

    def offset(self, name, word=0):
        return self.cols[name].start + word

    def image(self):
        img = np.full(self.size, FILL, np.uint32)
        for c in self.cols.values():
            if c.data is not None:
                img[c.start:c.end] = c.data
        return img

    def guard_mask(self):
        m = np.ones(self.size, bool)
        for c in self.cols.values():
            m[c.start:c.end] = False
        return m

    def _nearest(self, idx):
        """(column, word index relative to its first word) of the column nearest to slab word idx: negative = before it, >= words = past it"""
        best = None
        for c in self.cols.values():
            d = c.start - idx if idx < c.start else idx - (c.end - 1)
            if best is None or d < best[0]:
                best = (d, c)
        return best[1], idx - best[1].start

    def check(self, after, expect, limit=8):
        """after: the slab downloaded after the call; expect: {column: the oracle's words} for every column the call writes (in-place
        columns included).  Every other column must be what image() put there: an input byte-identical, an output nobody wrote still
        FILL.  Returns the list of violations, each naming the column and the word index; empty = the call respected the placement."""
        after = np.asarray(after, np.uint32)
        assert after.size == self.size
        errs = []
        bad = np.flatnonzero(self.guard_mask() & (after != FILL))
        for idx in bad[:limit]:
            c, w = self._nearest(int(idx))
            where = f"{-w} word(s) before its first word" if w < 0 else f"{w - c.words + 1} word(s) past its last word"
            errs.append(f"guard of column {c.name} overwritten at word index {w} ({where}): 0x{int(after[idx]):08x}")
        if len(bad) > limit:
            errs.append(f"... {len(bad)} guard words overwritten in all")
        for c in self.cols.values():
            got = after[c.start:c.end]
            if c.name in expect:
                want = np.ascontiguousarray(expect[c.name], dtype=np.uint32).reshape(-1)
                assert want.size == c.words, (c.name, want.size, c.words)
                d = np.flatnonzero(got != want)
                if d.size:
                    w = int(d[0])
                    note = " (still the fill value: never written)" if got[w] == FILL else ""
                    errs.append(f"output column {c.name} differs from the oracle at word index {w}: 0x{int(got[w]):08x} != 0x{int(want[w]):08x}{note}; {d.size} word(s) differ")
            else:
                want = c.data if c.data is not None else np.full(c.words, FILL, np.uint32)
                d = np.flatnonzero(got != want)
                if d.size:
                    w = int(d[0])
                    what = "input column" if c.data is not None else "untouched output column"
                    errs.append(f"{what} {c.name} changed at word index {w}: 0x{int(got[w]):08x} != 0x{int(want[w]):08x}; {d.size} word(s) differ")
        return errs


class Shifts:
    """The word offsets modulo 4 of the columns of one case.  word(): the next column the kernel touches word by word — column k of the
    case gets (s (k + 1)) mod 4, so a case with s != 0 mixes aligned and misaligned operands (what a host branch ORs together) and s = 0
    aligns everything.  wide(arg, align): a column of a W argument — the nearest offset the contract allows (0 for 16 bytes, 0 or 2 for
    8), or, in a refusal case, the forbidden offset for argument `arg` (column `index` of it)."""

    def __init__(self, s, refuse=None):
        self.s, self.k, self.refuse = s, 0, refuse

    def word(self):
        self.k += 1
        return (self.s * self.k) % 4

    def wide(self, arg, align, index=None):
        if self.refuse and self.refuse[0] == arg and (len(self.refuse) < 3 or self.refuse[2] is None or self.refuse[2] == index):
            return self.refuse[1]
        v = self.word()
        return v - v % (align // 4)


# ------------------------------------------------------------------------------------------------------------------ the table

Row = namedtuple("Row", "entry family cls cites sizes vector_from wide exempt_below note")
Wide = namedtuple("Wide", "arg bytes cite index")
TABLE = {}
BUILDERS = {}


def entry(name, family, cls, cites, sizes, vector_from=None, wide=(), exempt_below=None, note=""):
    """registers the classification row of a public entry and the builder of its cases"""
    def deco(fn):
        TABLE[name] = Row(name, family, cls, tuple(cites), tuple(sizes), vector_from, tuple(Wide(*w) for w in wide), exempt_below, note)
        BUILDERS[name] = fn
        return fn
    return deco


class Plan:
    """One case laid out: the arena, what the call must leave in it, what it must return to the host, and what the runner needs."""

    def __init__(self, **args):
        self.arena = Arena()
        self.expect, self.host, self.args = {}, {}, dict(args)

    def add(self, name, data=None, words=None, shift=0):
        return self.arena.add(name, data, words, shift)

    def slab(self, name, cols, shift):
        """n contiguous columns (a DeviceColumns view): one guarded slab"""
        return self.arena.add(name, np.stack([np.asarray(c, np.uint32) for c in cols]), None, shift)

    def out_slab(self, name, n_cols, log, shift):
        return self.arena.add(name, None, n_cols << log, shift)

    def want(self, name, cols):
        self.expect[name] = np.ascontiguousarray(np.stack([np.asarray(c, np.uint32) for c in cols]) if isinstance(cols, (list, tuple)) else cols, dtype=np.uint32).reshape(-1)


Case = namedtuple("Case", "entry log shift variant refuse")


def case_id(c):
    s = f"{c.entry}-L{c.log}-s{c.shift}"
    if c.variant:
        s += f"-{c.variant}"
    if c.refuse:
        s += f"-refuse-{c.refuse[0]}" + (f"{c.refuse[2]}" if len(c.refuse) > 2 and c.refuse[2] is not None else "") + f"+{c.refuse[1]}"
    return s


def build(case):
    """the Plan of a case: deterministic inputs, laid out, with the oracle's outputs"""
    seed = [abs(hash_name(case.entry)) % (1 << 31), case.log, case.shift, abs(hash_name(case.variant or ""))]
    rng = np.random.default_rng(seed)
    plan = BUILDERS[case.entry](case.log, Shifts(case.shift, case.refuse), rng, case.variant)
    plan.case = case
    if case.refuse:                      # nothing is launched: every column is what it was, every output still FILL
        plan.expect, plan.host = {}, {}
    return plan


def hash_name(s):
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % (1 << 61)
    return h


def m31(rng, *shape):
    return rng.integers(0, P, shape, dtype=np.uint32)


def nonzero31(rng, *shape):
    return rng.integers(1, P, shape, dtype=np.uint32)


def edge(cols):
    """the boundary words 0, 1, p - 1 in the first rows of every column"""
    cols = np.array(cols, np.uint32, copy=True)
    flat = cols.reshape(-1, cols.shape[-1])
    for c in range(flat.shape[0]):
        k = min(3, flat.shape[1])
        flat[c, :k] = np.roll(np.array([0, 1, P - 1], np.uint32), c)[:k]
    return cols


_TW = {}


def otw(root_log=16):
    if root_log not in _TW:
        _TW[root_log] = O.Twiddles(root_log)
    return _TW[root_log]


def channel_values(seed):
    """two circle points (8 words) and one secure felt out of the oracle's channel"""
    L = O.lib()
    ch = C.c_void_p(L.orc_channel_new())
    L.orc_channel_mix_u64(ch, seed)
    p1, p2, a = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(4, np.uint32)
    L.orc_get_random_point(ch, O.ptr(p1))
    L.orc_get_random_point(ch, O.ptr(p2))
    L.orc_channel_draw_secure_felt(ch, O.ptr(a))
    L.orc_channel_free(ch)
    return p1, p2, a


def contig(cols):
    return [np.ascontiguousarray(c, dtype=np.uint32) for c in cols]


# ------------------------------------------------------------------------------------------------------------------ transforms
TW_LOG = 15      # the device twiddle tree of the GPU tests: covers domains up to 2^16

_FFT_CITES = ("fft.hip:199 uint4 load of the tile", "fft.hip:228 uint4 store of the tile", "fft.hip:349 2^1/2^2 rows: fft_tiny_kernel, words", "fft.hip:238", "fft.hip:257",
              "fft13.hip:94 gload4 / gload2", "fft13.hip:389 gstore4")


@entry("nx_interpolate_batch", "transforms", "W", _FFT_CITES, sizes=(1, 2, 3, 5, 6, 13), exempt_below=3,
       wide=[("d_cols", 16, "fft.hip:199", 1)])
def _interpolate(log, sh, rng, variant):
    p = Plan(log=log, n_cols=2)
    vals = edge(m31(rng, 2, 1 << log))
    for k in range(2):         # a pointer list: each column guarded
        p.add(f"col{k}", vals[k], shift=sh.word() if log < 3 else sh.wide("d_cols", 16, k))
        p.want(f"col{k}", otw().interpolate(vals[k]))
    return p


@entry("nx_evaluate_batch", "transforms", "W", _FFT_CITES + ("fft.hip:366 an output of 2^1/2^2 rows: fft_tiny_kernel",), sizes=(1, 2, 3, 5, 6, 13), exempt_below=2,
       wide=[("d_polys", 16, "fft.hip:199", 1), ("d_out", 16, "fft.hip:228", 0)], note="log_expand 1; a 2-word source is read word by word, fft.hip:200")
def _evaluate(log, sh, rng, variant):
    p = Plan(log=log, n_cols=2, log_expand=1)
    coef = edge(m31(rng, 2, 1 << log))
    for k in range(2):
        p.add(f"poly{k}", coef[k], shift=sh.word() if log < 2 else sh.wide("d_polys", 16, k))
    for k in range(2):
        p.add(f"out{k}", words=2 << log, shift=sh.word() if log + 1 < 3 else sh.wide("d_out", 16, k))
        p.want(f"out{k}", otw().evaluate(coef[k], log + 1))
    return p


def _lde_plan(log, sh, rng, n_cols=2, entry_name="nx_lde_batch"):
    p = Plan(log=log, n_cols=n_cols, log_blowup=1)
    vals = edge(m31(rng, n_cols, 1 << log))
    coef = [otw().interpolate(v) for v in vals]
    for k in range(n_cols):     # in place: evaluations on entry, coefficients on return (documented)
        p.add(f"col{k}", vals[k], shift=sh.word() if log < 2 else sh.wide("d_cols", 16, k))
        p.want(f"col{k}", coef[k])
    ldes = [otw().evaluate(c, log + 1) for c in coef]
    for k in range(n_cols):
        p.add(f"lde{k}", words=2 << log, shift=sh.word() if log + 1 < 3 else sh.wide("d_lde", 16, k))
        p.want(f"lde{k}", ldes[k])
    p.args["ldes"] = ldes
    return p


@entry("nx_lde_batch", "transforms", "W", _FFT_CITES + ("prover.hip:248 lde_batch_from", "fft.hip:432 fused middle launch from 2^14 rows"),
       sizes=(1, 2, 3, 5, 6, 13, 14), exempt_below=2, wide=[("d_cols", 16, "fft.hip:199", 1), ("d_lde", 16, "fft.hip:228", 0)],
       note="log_blowup 1; in place: d_cols holds the coefficients on return")
def _lde_batch(log, sh, rng, variant):
    return _lde_plan(log, sh, rng)


@entry("nx_lde_commit", "transforms", "W", _FFT_CITES + ("prover.hip:1797 nx_lde_batch then nx_merkle_commit",), sizes=(1, 2, 3, 6), exempt_below=2,
       wide=[("d_cols", 16, "fft.hip:199", 1), ("d_lde", 16, "fft.hip:228", 0)], note="the refusal is nx_lde_batch's")
def _lde_commit(log, sh, rng, variant):
    p = _lde_plan(log, sh, rng, n_cols=3)
    p.host["root"] = O.merkle_commit(p.args["ldes"], O.HASH_STD)
    return p


@entry("nx_commit_root", "transforms", "W", _FFT_CITES + ("merkle.hip:1101 nx_lde_batch per size", "merkle.hip:1121",), sizes=(1, 5), exempt_below=2,
       wide=[("d_cols", 16, "fft.hip:199", 2)], note="mixed sizes (log 5: columns of 2^5, 2^3, 2^1 rows; log 1: 2^1 only); consumed: coefficients on return")
def _commit_root(log, sh, rng, variant):
    logs = [1, 1, 1] if log == 1 else [5, 3, 5, 1, 1, 3]
    p = Plan(logs=logs, log_blowup=1)
    vals = [edge(m31(rng, 1, 1 << l))[0] for l in logs]
    work = [v.copy() for v in vals]
    _, root = O.lde_commit(work, 1, O.HASH_STD, threads=1)
    for k, l in enumerate(logs):
        p.add(f"col{k}", vals[k], shift=sh.word() if l < 2 else sh.wide("d_cols", 16, k))
        p.want(f"col{k}", work[k])
    p.host["root"] = root
    return p


# ------------------------------------------------------------------------------------------------------------------ Merkle

def _oracle_layer(log, prev, cols, mode):
    out = np.zeros(8 << log, np.uint32)
    cs = contig(cols)
    O.lib().orc_commit_on_layer(log, O.ptr(prev) if prev is not None else None, O.ptr_array(cs) if cs else None, C.c_size_t(len(cs)), mode, O.ptr(out))
    return out


FUSED_LOG = 12     # merkle.hip:601 FUSED_MIN_LOG: the GPU test lowers the context option "merkle.fused" (default 21) to it


@entry("nx_merkle_commit", "merkle", "B", ("merkle.hip:995 aligned16 selects merkle_commit_fused", "merkle.hip:650 gld4 of 4 rows", "merkle.hip:82 load_ptrs16: words"),
       sizes=(0, 1, 2, 3, 5, 6, FUSED_LOG), vector_from="2^12 rows (FUSED_MIN_LOG, context option merkle.fused lowered to 12), 1 .. 4 columns of one size",
       note="both hash modes; variant mixed: columns of 2^log, 2^(log-2), 2^0 rows")
def _merkle_commit(log, sh, rng, variant):
    mode = 1 if "raw0" in variant else 0
    if log == FUSED_LOG:
        logs = [log, log]
    elif "mixed" in variant:
        logs = [log, max(log - 2, 0), log, 0, max(log - 2, 0)]
    else:
        logs = [log] * 3
    p = Plan(logs=logs, mode=mode)
    cols = [m31(rng, 1 << l) for l in logs]
    for k, c in enumerate(cols):
        p.add(f"col{k}", c, shift=sh.word())
    root, layers = O.merkle_commit(cols, mode, want_layers=True)
    p.host["root"], p.host["layers"] = root, layers
    return p


@entry("nx_merkle_commit_on_layer", "merkle", "W", ("merkle.hip:159 gld4 of the two child nodes", "merkle.hip:173 uint4 stores of the node", "merkle.hip:82 columns: words"),
       sizes=(0, 1, 2, 3, 5, 6), wide=[("d_prev_layer", 16, "merkle.hip:159", None), ("d_out", 16, "merkle.hip:173", None)],
       note="a node is 8 words: never shorter than the access; the injected columns are read word by word and are shifted")
def _commit_on_layer(log, sh, rng, variant):
    mode = 1 if "raw0" in variant else 0
    n_cols = 0 if "nodes" in variant else 3
    p = Plan(log=log, mode=mode, n_cols=n_cols, has_prev="leaf" not in variant)
    prev = None
    if p.args["has_prev"]:
        prev = rng.integers(0, 1 << 32, 16 << log, dtype=np.uint64).astype(np.uint32)
        p.add("prev", prev, shift=sh.wide("d_prev_layer", 16))
    cols = [m31(rng, 1 << log) for _ in range(n_cols)]
    for k, c in enumerate(cols):
        p.add(f"col{k}", c, shift=sh.word())
    p.add("out", words=8 << log, shift=sh.wide("d_out", 16))
    p.want("out", _oracle_layer(log, prev, cols, mode))
    return p


@entry("nx_merkle_leaf_chain", "merkle", "W", ("merkle.hip:263 uint4 loads of the state", "merkle.hip:277 uint4 stores of the state", "merkle.hip:82 columns: words"),
       sizes=(1, 2, 3, 5, 6), wide=[("d_state_in", 16, "merkle.hip:263", None), ("d_state_out", 16, "merkle.hip:277", None)],
       note="two shards (16 + 4 columns) over one state buffer (in and out may alias); the columns are shifted")
def _leaf_chain(log, sh, rng, variant):
    mode = 1 if "raw0" in variant else 0
    p = Plan(log=log, mode=mode, n_cols=20)
    cols = [m31(rng, 1 << log) for _ in range(20)]
    for k, c in enumerate(cols):
        p.add(f"col{k}", c, shift=sh.word())
    refuse_in = sh.refuse and sh.refuse[0] == "d_state_in"
    p.add("state", words=8 << log, shift=sh.wide("d_state_in" if refuse_in else "d_state_out", 16))
    p.want("state", _oracle_layer(log, None, cols, mode))
    return p


@entry("nx_merkle_from_leaves", "merkle", "B", ("merkle.hip:1174 nx_copy of the digests", "ctx.hip:555 nx_copy: copy_kernel (uint4) or hipMemcpyAsync"),
       sizes=(0, 1, 2, 3, 5, 6), vector_from="every size (8 words per digest: n_words & 3 == 0), decided by the pointer alone")
def _from_leaves(log, sh, rng, variant):
    mode = 1 if "raw0" in variant else 0
    p = Plan(log=log, mode=mode)
    leaves = rng.integers(0, 1 << 32, 8 << log, dtype=np.uint64).astype(np.uint32)
    p.add("leaves", leaves, shift=sh.word())
    layers, cur = [leaves], leaves
    for l in range(log - 1, -1, -1):
        cur = _oracle_layer(l, cur, [], mode)
        layers.append(cur)
    p.host["layers"] = np.concatenate(layers)
    p.host["root"] = layers[-1]
    return p


# ------------------------------------------------------------------------------------------------------------------ PCS

@entry("nx_eval_at_points", "pcs", "S", ("pcs.hip:42 gld per coefficient", "pcs.hip:62"), sizes=(0, 1, 2, 3, 5, 6, 11),
       note="2^11: the first size with more than one high-table row (EVAL_LOG_LO = 10)")
def _eval_at_points(log, sh, rng, variant):
    p = Plan(log=log, n_cols=3, idx=[0, 1, 2, 0, 2])
    polys = edge(m31(rng, 3, 1 << log))
    for k in range(3):
        p.add(f"poly{k}", polys[k], shift=sh.word())
    p1, p2, _ = channel_values(log + 77)
    p.args["points"] = [p1, p1, p1, p2, p2]
    p.host["values"] = np.stack([O.eval_at_point(polys[i], pt) for i, pt in zip(p.args["idx"], p.args["points"])])
    return p


def _quotient_plan(log, sh, rng):
    n_cols = 6
    p = Plan(log=log, n_cols=n_cols)
    cols = edge(m31(rng, n_cols, 1 << log))
    for k in range(n_cols):
        p.add(f"col{k}", cols[k], shift=sh.word() if log < 2 else sh.wide("d_cols", 16, k))
    p1, p2, alpha = channel_values(log + 5)
    b1 = [(c, m31(rng, 4)) for c in range(n_cols)]       # 6 entries: one unrolled group of 4 + 2 in the tail loop
    b2 = [(c, m31(rng, 4)) for c in (0, 3)]
    pts, counts = np.concatenate([p1, p2]), np.array([len(b1), len(b2)], np.int32)
    cidx, vals = np.array([c for c, _ in b1 + b2], np.int32), np.concatenate([v for _, v in b1 + b2])
    outs = [np.zeros(1 << log, np.uint32) for _ in range(4)]
    O.lib().orc_accumulate_quotients(log, O.ptr_array(contig(cols)), n_cols, O.ptr(alpha), 2, O.ptr(pts), O.ptr(counts), O.ptr(cidx), O.ptr(vals), 4, O.ptr_array(outs))
    for q in range(4):
        p.add(f"out{q}", words=1 << log, shift=sh.word() if log < 2 else sh.wide("d_out4", 16, q))
        p.want(f"out{q}", outs[q])
    p.args.update(alpha=alpha, points=pts, counts=counts.astype(np.uint32), cidx=cidx.astype(np.uint32), values=vals)
    return p


_QUOT_CITES = ("pcs.hip:151 gld4 of 4 rows of a column", "pcs.hip:166", "pcs.hip:184 uint4 stores", "pcs.hip:637 2 rows: quotient_small_kernel, words", "pcs.hip:319", "pcs.hip:325")


@entry("nx_accumulate_quotients", "pcs", "W", _QUOT_CITES, sizes=(1, 2, 3, 5, 6, 11), exempt_below=2,
       wide=[("d_cols", 16, "pcs.hip:151", 1), ("d_out4", 16, "pcs.hip:184", 2)], note="2^11: more than one block")
def _quotients(log, sh, rng, variant):
    return _quotient_plan(log, sh, rng)


@entry("nx_accumulate_quotients_partial", "pcs", "W", _QUOT_CITES, sizes=(1, 2, 3, 6), exempt_below=2,
       wide=[("d_cols", 16, "pcs.hip:151", 1), ("d_out4", 16, "pcs.hip:184", 2)], note="entry_local NULL, line terms included: nx_accumulate_quotients")
def _quotients_partial(log, sh, rng, variant):
    return _quotient_plan(log, sh, rng)


def _fold_plan(log, sh, rng, circle, alias=False):
    """src: 4 coordinate columns of 2^log words packed at ptr + k len (the Rust shim's coord_ptr): 8-byte aligned from 2 words on"""
    p = Plan(log=log, alias=alias)
    src = edge(m31(rng, 4, 1 << log))
    _, _, alpha = channel_values(log + 9)
    p.args["alpha"] = alpha
    p.slab("src", src, sh.wide("d_src4", 8, 0))
    if circle:
        dst0 = edge(m31(rng, 4, 1 << (log - 1)))
        ref = contig(dst0.copy())
        O.lib().orc_fold_circle_into_line(O.ptr_array(ref), O.ptr_array(contig(src)), log, O.ptr(alpha))
        p.slab("dst", dst0, sh.word())           # accumulating destination (documented): dst = dst alpha^2 + fold(src)
    else:
        ref = [np.zeros(1 << (log - 1), np.uint32) for _ in range(4)]
        O.lib().orc_fold_line_dom(O.ptr_array(contig(src)), log, 0, O.ptr(alpha), O.ptr_array(ref))
        p.out_slab("dst", 4, log - 1, sh.word())
    p.want("dst", ref)
    return p


@entry("nx_fold_circle_into_line", "pcs", "W", ("pcs.hip:354 uint2 loads of the pair", "pcs.hip:360 dst: words"), sizes=(1, 2, 3, 5, 6, 9),
       wide=[("d_src4", 8, "pcs.hip:354", 0)], note="a 2-word column is as long as the access: no exemption; dst (word access, accumulating) is shifted; src at 0 or 2 words")
def _fold_circle(log, sh, rng, variant):
    return _fold_plan(log, sh, rng, True)


@entry("nx_fold_line", "pcs", "W", ("pcs.hip:370 uint2 loads of the pair", "pcs.hip:375 dst: words"), sizes=(1, 2, 3, 5, 6, 9),
       wide=[("d_src4", 8, "pcs.hip:370", 0)], note="dst (word access) is shifted; src at 0 or 2 words")
def _fold_line(log, sh, rng, variant):
    return _fold_plan(log, sh, rng, False)


@entry("nx_fri_decompose", "pcs", "S", ("backend_ops.hip:44 s.c[q][i]", "backend_ops.hip:84 g.c[q][i]"), sizes=(1, 2, 3, 5, 6, 13), note="2^13: two blocks of partial sums")
def _decompose(log, sh, rng, variant):
    p = Plan(log=log)
    src = edge(m31(rng, 4, 1 << log))
    ref, lam = [np.zeros(1 << log, np.uint32) for _ in range(4)], np.zeros(4, np.uint32)
    O.lib().orc_fri_decompose(O.ptr_array(contig(src)), log, O.ptr_array(ref), O.ptr(lam))
    p.slab("src", src, sh.word())
    p.out_slab("g", 4, log, sh.word())
    p.want("g", ref)
    p.host["lambda"] = lam
    return p


# ------------------------------------------------------------------------------------------------------------------ field utilities

@entry("nx_secure_accumulate", "field", "S", ("air.hip:166 d[i] = m_add(d[i], s[i])",), sizes=(0, 1, 2, 3, 5, 6, 9), note="accumulating destination (documented)")
def _secure_accumulate(log, sh, rng, variant):
    p = Plan(log=log)
    a, b = edge(m31(rng, 4, 1 << log)), edge(m31(rng, 4, 1 << log))[::-1]
    ref = contig(a.copy())
    O.lib().orc_secure_accumulate(O.ptr_array(ref), O.ptr_array(contig(b)), C.c_size_t(1 << log))
    p.slab("dst", a, sh.word())
    p.slab("src", b, sh.word())
    p.want("dst", ref)
    return p


ODD_SIZES = (1, 3, 4, 37, 64, 300)       # `log` of the flat entries indexes this list: word counts, not powers of two


@entry("nx_batch_inverse_m31", "field", "S", ("backend_ops.hip:19 dst[i] = m_inv(src[i])",), sizes=range(len(ODD_SIZES)), note="sizes are word counts ODD_SIZES[log]; variant alias: dst == src (documented)")
def _inv_m31(log, sh, rng, variant):
    n = ODD_SIZES[log]
    p = Plan(n=n, alias="alias" in variant)
    v = nonzero31(rng, n)
    v[:min(2, n)] = np.array([1, P - 1], np.uint32)[:min(2, n)]
    ref = np.zeros(n, np.uint32)
    O.lib().orc_batch_inverse_m31(O.ptr(v), O.ptr(ref), C.c_size_t(n))
    p.add("src", v, shift=sh.word())
    if p.args["alias"]:
        p.want("src", ref)
    else:
        p.add("dst", words=n, shift=sh.word())
        p.want("dst", ref)
    return p


@entry("nx_batch_inverse_qm31", "field", "S", ("backend_ops.hip:25", "backend_ops.hip:26"), sizes=(0, 1, 2, 3, 5, 6), note="variant alias: dst == src (documented)")
def _inv_qm31(log, sh, rng, variant):
    p = Plan(log=log, alias="alias" in variant)
    v = m31(rng, 4, 1 << log)
    v[0] |= 1
    ref = [np.zeros(1 << log, np.uint32) for _ in range(4)]
    O.lib().orc_batch_inverse_qm31(O.ptr_array(contig(v)), O.ptr_array(ref), C.c_size_t(1 << log))
    p.slab("src", v, sh.word())
    if p.args["alias"]:
        p.want("src", ref)
    else:
        p.out_slab("dst", 4, log, sh.word())
        p.want("dst", ref)
    return p


@entry("nx_m31_add_into", "field", "S", ("ctx.hip:275 m31_add_into_kernel: words",), sizes=range(len(ODD_SIZES)))
def _add_into(log, sh, rng, variant):
    n = ODD_SIZES[log]
    p = Plan(n=n)
    a, b = edge(m31(rng, 1, n))[0], edge(m31(rng, 1, n))[0][::-1].copy()
    p.add("dst", a, shift=sh.word())
    p.add("src", b, shift=sh.word())
    p.want("dst", ((a.astype(np.uint64) + b) % P).astype(np.uint32))
    return p


@entry("nx_m31_widen", "field", "W", ("ctx.hip:277 m31_widen_kernel: u64 stores, src words", "ctx.hip:278"), sizes=range(len(ODD_SIZES)),
       wide=[("d_dst", 8, "ctx.hip:277", None)], note="src (word access) is shifted; dst at 0 or 2 words")
def _widen(log, sh, rng, variant):
    n = ODD_SIZES[log]
    p = Plan(n=n)
    a = edge(m31(rng, 1, n))[0]
    p.add("src", a, shift=sh.word())
    p.add("dst", words=2 * n, shift=sh.wide("d_dst", 8))
    p.want("dst", a.astype(np.uint64).view(np.uint32))
    return p


@entry("nx_m31_narrow", "field", "W", ("ctx.hip:280 m31_narrow_kernel: u64 loads, dst words", "ctx.hip:281"), sizes=range(len(ODD_SIZES)),
       wide=[("d_src", 8, "ctx.hip:280", None)], note="dst (word access) is shifted; src at 0 or 2 words; sums of up to 2^33 p reduced mod p")
def _narrow(log, sh, rng, variant):
    n = ODD_SIZES[log]
    p = Plan(n=n)
    a = rng.integers(0, (1 << 33) * P, n, dtype=np.uint64)
    a[:min(3, n)] = np.array([0, P, (1 << 64) - 1], np.uint64)[:min(3, n)]
    p.add("src", a.view(np.uint32), shift=sh.wide("d_src", 8))
    p.add("dst", words=n, shift=sh.word())
    p.want("dst", (a % np.uint64(P)).astype(np.uint32))
    return p


# ------------------------------------------------------------------------------------------------------------------ layout and copies

def _bitrev_perm(log):
    i = np.arange(1 << log)
    r = np.zeros_like(i)
    for b in range(log):
        r |= ((i >> b) & 1) << (log - 1 - b)
    return r


@entry("nx_bit_reverse", "layout", "S", ("fft.hip:464 bit_reverse_kernel: words",), sizes=(0, 1, 2, 3, 5, 6, 9), note="in place (documented)")
def _bit_reverse(log, sh, rng, variant):
    p = Plan(log=log)
    v = m31(rng, 1 << log)
    ref = v.copy()
    O.lib().orc_bit_reverse(O.ptr(ref), log)
    assert np.array_equal(ref, v[_bitrev_perm(log)])
    p.add("col", v, shift=sh.word())
    p.want("col", ref)
    return p


@entry("nx_bit_reverse_secure", "layout", "S", ("backend_ops.hip:137 nx_bit_reverse per coordinate",), sizes=(0, 1, 2, 3, 5, 6), note="in place (documented)")
def _bit_reverse_secure(log, sh, rng, variant):
    p = Plan(log=log)
    v = m31(rng, 4, 1 << log)
    p.slab("col4", v, sh.word())
    p.want("col4", v[:, _bitrev_perm(log)])
    return p


@entry("nx_finalize_columns", "layout", "S", ("fft.hip:476 finalize_kernel: words",), sizes=(1, 2, 3, 5, 6, 9))
def _finalize(log, sh, rng, variant):
    p = Plan(log=log, n_cols=3)
    v = m31(rng, 3, 1 << log)
    for k in range(3):
        p.add(f"src{k}", v[k], shift=sh.word())
    for k in range(3):
        p.add(f"dst{k}", words=1 << log, shift=sh.word())
        p.want(f"dst{k}", O.finalize_column(v[k]))
    return p


@entry("nx_upload_coset_order", "layout", "S", ("fft.hip:747 finalize_kernel behind the copy into a temporary", "fft.hip:476"), sizes=(1, 2, 3, 5, 6))
def _upload_coset(log, sh, rng, variant):
    p = Plan(log=log)
    v = m31(rng, 1 << log)
    p.args["host"] = v
    p.add("dst", words=1 << log, shift=sh.word())
    p.want("dst", O.finalize_column(v))
    return p


@entry("nx_upload_columns", "layout", "S", ("fft.hip:740 hipMemcpyAsync into the column", "fft.hip:747 finalize_kernel: words"), sizes=(1, 2, 3, 5, 6),
       note="variants: coset order (permuted on the device) and circle order (copied as it is)")
def _upload_columns(log, sh, rng, variant):
    coset = "coset" in variant
    p = Plan(log=log, n_cols=3, coset=coset)
    v = m31(rng, 3, 1 << log)
    p.args["host"] = v
    for k in range(3):
        p.add(f"dst{k}", words=1 << log, shift=sh.word())
        p.want(f"dst{k}", O.finalize_column(v[k]) if coset else v[k])
    return p


@entry("nx_upload_columns_narrow", "layout", "B", ("fft.hip:783 vec = n >= per_lane && dst 16-byte aligned", "fft.hip:496 widen_kernel: gst4", "fft.hip:489 or words", "fft.hip:487 coset order: words"),
       sizes=(1, 2, 3, 4, 5, 6), vector_from="2^4 rows of u8 / 2^3 rows of u16 (per_lane = 16 / width values), circle order")
def _upload_narrow(log, sh, rng, variant):
    coset = "coset" in variant
    p = Plan(log=log, coset=coset)
    host = [rng.integers(0, 256, 1 << log, dtype=np.uint8), rng.integers(0, 1 << 16, 1 << log, dtype=np.uint16), m31(rng, 1 << log)]
    host[0][0], host[1][0] = 255, 65535
    p.args["host"] = host
    for k, h in enumerate(host):
        p.add(f"dst{k}", words=1 << log, shift=sh.word())
        w = h.astype(np.uint32)
        p.want(f"dst{k}", O.finalize_column(w) if coset else w)
    return p


COPY_SIZES = (1, 3, 4, 8, 64, 257, 1024)


@entry("nx_copy", "layout", "B", ("ctx.hip:555 (n_words & 3) or a misaligned pointer: hipMemcpyAsync", "ctx.hip:270 else copy_kernel (uint4)"), sizes=range(len(COPY_SIZES)),
       vector_from="every multiple of 4 words (n_words & 3 == 0)", note="sizes are word counts COPY_SIZES[log]; copy_columns (ctx.hip:326-328: n_cols >= 4, the same test of the pointers) is internal: the existing host-commit tests reach it")
def _copy(log, sh, rng, variant):
    n = COPY_SIZES[log]
    p = Plan(n=n)
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    p.add("src", v, shift=sh.word())
    p.add("dst", words=n, shift=sh.word())
    p.want("dst", v)
    return p


# ------------------------------------------------------------------------------------------------------------------ logup

def _alpha_powers(rng, k):
    alpha = m31(rng, 4)
    ap = [np.array([1, 0, 0, 0], np.uint32)]
    for _ in range(k - 1):
        ap.append(O.qm31_mul(ap[-1], alpha))
    return np.stack(ap)


_LOGUP_SIZES = (0, 1, 2, 3, 5, 6, 9)
MINUS_ONE = (P - 1, 0, 0, 0)


@entry("nx_logup_combine", "logup", "S", ("logup.hip:30 cols.col(k)[r]", "logup.hip:35 out.c[q][r]"), sizes=_LOGUP_SIZES, note="2^9: two blocks")
def _logup_combine(log, sh, rng, variant):
    p = Plan(log=log, n_cols=5)
    t = edge(m31(rng, 5, 1 << log))
    ap, z = _alpha_powers(rng, 5), m31(rng, 4)
    p.args.update(alphas=ap, z=z)
    for k in range(5):
        p.add(f"tuple{k}", t[k], shift=sh.word())
    p.out_slab("out", 4, log, sh.word())
    p.want("out", O.logup_combine(list(t), ap, z))
    return p


@entry("nx_logup_finalize_col", "logup", "S", ("logup.hip:41 mult[r]", "logup.hip:42 den.c[q][r]", "logup.hip:54 prev", "logup.hip:55 out"), sizes=_LOGUP_SIZES, note="two merged fractions on a previous column; variant alias: out == prev (documented)")
def _logup_finalize_col(log, sh, rng, variant):
    alias = "alias" in variant
    p = Plan(log=log, alias=alias)
    n = 1 << log
    den_a, den_b = m31(rng, 4, n), m31(rng, 4, n)
    den_a[0] |= 1
    den_b[0] |= 1
    mult_a, mult_b, prev = rng.integers(0, 1 << 16, n, dtype=np.uint32), rng.integers(0, 1 << 16, n, dtype=np.uint32), m31(rng, 4, n)
    ref = O.logup_finalize_col(list(den_a), scale_a=MINUS_ONE, mult_a=mult_a, den_b=list(den_b), mult_b=mult_b, prev=list(prev))
    p.slab("den_a", den_a, sh.word())
    p.slab("den_b", den_b, sh.word())
    p.add("mult_a", mult_a, shift=sh.word())
    p.add("mult_b", mult_b, shift=sh.word())
    p.slab("prev", prev, sh.word())
    if alias:
        p.want("prev", ref)
    else:
        p.out_slab("out", 4, log, sh.word())
        p.want("out", ref)
    return p


def _fracs(rng, n, widths):
    """fractions over tuples of the given widths: multiplicity on every second, numerator scale +-1"""
    out = []
    for f, w in enumerate(widths):
        out.append(dict(tuple=edge(m31(rng, w, n)), alphas=None, mult=rng.integers(0, 1 << 16, n, dtype=np.uint32) if f % 2 else None,
                        scale=MINUS_ONE if f % 3 == 1 else (1, 0, 0, 0)))
    return out


def _place_fracs(p, sh, fracs, ap, z):
    for f, fr in enumerate(fracs):
        fr["alphas"], fr["z"] = ap[:len(fr["tuple"])], z
        fr["tuple_names"] = [p.add(f"f{f}t{k}", c, shift=sh.word()) for k, c in enumerate(fr["tuple"])]
        fr["mult_name"] = p.add(f"f{f}m", fr["mult"], shift=sh.word()) if fr["mult"] is not None else None


def _chain(fracs, ap, z, groups):
    """column j = the sum of the fractions of groups[0 .. j] (the oracle's combine + finalize_col chained through prev)"""
    cols, prev = [], None
    for g in groups:
        fs = list(g)
        while fs:
            a = fracs[fs.pop(0)]
            da = O.logup_combine(list(a["tuple"]), ap[:len(a["tuple"])], z)
            if fs:
                b = fracs[fs.pop(0)]
                db = O.logup_combine(list(b["tuple"]), ap[:len(b["tuple"])], z)
                prev = O.logup_finalize_col(da, scale_a=a["scale"], mult_a=a["mult"], den_b=db, scale_b=b["scale"], mult_b=b["mult"], prev=prev)
            else:
                prev = O.logup_finalize_col(da, scale_a=a["scale"], mult_a=a["mult"], prev=prev)
        cols.append(prev)
    return cols


@entry("nx_logup_col", "logup", "S", ("logup.hip:67 f.cols.col(k)[r]", "logup.hip:77 mult[r]", "logup.hip:84 prev", "logup.hip:85 out"), sizes=_LOGUP_SIZES, note="two fractions on a previous column; variant alias: out == prev (documented)")
def _logup_col(log, sh, rng, variant):
    alias = "alias" in variant
    p = Plan(log=log, alias=alias)
    n = 1 << log
    fracs, ap, z = _fracs(rng, n, (1, 5)), _alpha_powers(rng, 5), m31(rng, 4)
    _place_fracs(p, sh, fracs, ap, z)
    prev = m31(rng, 4, n)
    ref = _chain(fracs, ap, z, [(0, 1)])[0]
    ref = [((np.asarray(r, np.uint64) + pv) % P).astype(np.uint32) for r, pv in zip(ref, prev)]
    p.slab("prev", prev, sh.word())
    p.args["fracs"] = fracs
    if alias:
        p.want("prev", ref)
    else:
        p.out_slab("out", 4, log, sh.word())
        p.want("out", ref)
    return p


def _logup_cols_plan(log, sh, rng, widths, groups):
    p = Plan(log=log, n_logup=len(groups))
    fracs, ap, z = _fracs(rng, 1 << log, widths), _alpha_powers(rng, max(widths)), m31(rng, 4)
    _place_fracs(p, sh, fracs, ap, z)
    p.args["fracs"] = fracs
    for j, col in enumerate(_chain(fracs, ap, z, groups)):
        p.out_slab(f"out{j}", 4, log, sh.word())
        p.want(f"out{j}", col)
    return p


@entry("nx_logup_cols", "logup", "S", ("logup.hip:119 gld of the multiplicity (a fraction without one reads and drops a word of out[0])", "logup.hip:129 gld of the tuple columns", "logup.hip:156", "logup.hip:183 gst"),
       sizes=_LOGUP_SIZES, note="9 fractions: one full group of 8 and a ragged one")
def _logup_cols(log, sh, rng, variant):
    widths = (1, 2, 3, 1, 4, 1, 2, 5, 3)
    return _logup_cols_plan(log, sh, rng, widths, [(f,) for f in range(len(widths))])


@entry("nx_logup_cols_batched", "logup", "S", ("logup.hip:119 logup_cols_kernel", "logup.hip:129", "logup.hip:183"), sizes=(1, 2, 3, 5, 6), note="NULL batching (pairs, odd count) and a non-monotone batching")
def _logup_cols_batched(log, sh, rng, variant):
    widths = (1, 2, 3, 1, 4)
    if "explicit" in variant:
        batching = [2, 0, 1, 1, 0]
        p = _logup_cols_plan(log, sh, rng, widths, [[f for f in range(5) if batching[f] == j] for j in range(3)])
        p.args["batching"] = batching
    else:
        p = _logup_cols_plan(log, sh, rng, widths, [(0, 1), (2, 3), (4,)])
        p.args["batching"] = None
    return p


SCAN_TILED_LOG = 13    # logup.hip:293 SC_MIN_LOG


@entry("nx_logup_finalize_last", "logup", "S", ("logup.hip:209 logup_scan_local_kernel: col.c[q][pos]", "logup.hip:232", "logup.hip:315 logup_scan_tile_kernel: gld", "logup.hip:342 gst", "logup.hip:363"),
       sizes=(1, 2, 3, 5, 6, SCAN_TILED_LOG), note="in place (documented); 2^13: the first size of the tiled scan (logup.hip:523)")
def _finalize_last(log, sh, rng, variant):
    p = Plan(log=log)
    v = m31(rng, 4, 1 << log)
    last, claimed = O.logup_finalize_last(list(v))
    p.slab("col4", v, sh.word())
    p.want("col4", last)
    p.host["claimed"] = claimed
    return p


@entry("nx_logup_finalize_last_batch", "logup", "S", ("logup.hip:534 the same kernels, blockIdx.y = column", "logup.hip:539"), sizes=(1, 2, 3, 6, SCAN_TILED_LOG), note="three secure columns, in place")
def _finalize_last_batch(log, sh, rng, variant):
    p = Plan(log=log, n=3)
    claimed = []
    for j in range(3):
        v = m31(rng, 4, 1 << log)
        last, cs = O.logup_finalize_last(list(v))
        p.slab(f"col4_{j}", v, sh.word())
        p.want(f"col4_{j}", last)
        claimed.append(cs)
    p.host["claimed"] = np.stack(claimed)
    return p


def relation_fraction_program(log):
    """the lookup-heavy example component of tests/air_examples.py: 5 relation entries, expressions and a next-row read"""
    import nexus_zkvm_amd.air_program as ap
    import air_examples as AE
    rng = np.random.default_rng(4242)
    z, alpha = m31(rng, 4), m31(rng, 4)
    return AE.relation_program(ap, z, alpha, (0, 0, 0, 0), "pairs").build_logup(), AE.relation_main_trace(log, 500 + log)[1]


@entry("nx_logup_program", "logup", "S", ("air_jit.hip:1067 generated loads G(cols[c])[row]: words", "air_jit.hip:1081", "air_jit.hip:1052 out[..][r]", "air_jit.hip:50 G: a u32 pointer"), sizes=(2, 3, 5, 6),
       note="one recorded program (air_examples.relation_program), compiled once per context")
def _logup_program(log, sh, rng, variant):
    frac, fin = relation_fraction_program(log)
    p = Plan(log=log, program=frac, n_in=len(fin))
    for k, c in enumerate(fin):
        p.add(f"col{k}", c, shift=sh.word())
    want = O.logup_program(frac, fin + [None] * (4 * frac.n_logup_cols), log, frac.n_logup_cols)
    for j, col in enumerate(want):
        for q in range(4):       # every coordinate column its own pointer: guarded one by one
            p.add(f"out{j}_{q}", words=1 << log, shift=sh.word())
            p.want(f"out{j}_{q}", col[q])
    return p


MULT_TILE_LOG = 12     # multiplicity.hip:27 MULT_TILE = 4096 rows


@entry("nx_logup_multiplicities", "logup", "B", ("multiplicity.hip:254 vec = n >= MULT_TILE && aligned", "internal.h:198 gld4_guarded", "multiplicity.hip:61", "multiplicity.hip:173 table / d_mult: words"),
       sizes=(0, 1, 3, 6, MULT_TILE_LOG), vector_from="2^12 rows of a use (MULT_TILE)")
def _multiplicities(log, sh, rng, variant):
    log_table, n = 4, 1 << log
    p = Plan(log=log, log_table=log_table, key_bits=[2, 2])
    perm = rng.permutation(1 << log_table)
    table = [(perm & 3).astype(np.uint32), (perm >> 2).astype(np.uint32)]
    vals = [rng.integers(0, 4, n, dtype=np.uint32), rng.integers(0, 4, n, dtype=np.uint32)]
    weight = m31(rng, n)
    for k in range(2):
        p.add(f"table{k}", table[k], shift=sh.word())
    for k in range(2):
        p.add(f"val{k}", vals[k], shift=sh.word())
    p.add("weight", weight, shift=sh.word())
    # second use without weights, half as long: its rows count 1 each
    n2 = max(n // 2, 1)
    v2 = [rng.integers(0, 4, n2, dtype=np.uint32), rng.integers(0, 4, n2, dtype=np.uint32)]
    counts = np.zeros(1 << log_table, np.uint64)
    np.add.at(counts, (vals[0] | (vals[1] << 2)).astype(np.int64), weight.astype(np.uint64))
    np.add.at(counts, (v2[0] | (v2[1] << 2)).astype(np.int64), 1)
    for k in range(2):
        p.add(f"second{k}", v2[k], shift=sh.word())
    p.args["log2"] = max(log - 1, 0)
    p.add("mult", words=1 << log_table, shift=sh.word())
    p.want("mult", (counts % P).astype(np.uint32)[perm])
    return p


# ------------------------------------------------------------------------------------------------------------------ AIR

def constraint_program():
    """a small recorded program with every load form: base columns at offsets -1 / 0 / +1, a secure column, base and secure constraints"""
    import nexus_zkvm_amd.air_program as ap
    pb = ap.ProgramBuilder()
    a, a1 = pb.next_trace_mask(0, (0, 1))
    (b,) = pb.next_trace_mask(1, (-1,))
    (c,) = pb.next_trace_mask(2)
    s0, s1 = pb.next_secure_mask(3, (0, 1))
    e = pb.econst([5, 6, 7, 8])
    pb.add_constraint(a * b - c + 3)
    pb.add_constraint(s0 * a1 + e - s1)
    pb.add_constraint((s0 + s1) * (s0 - e) + b)
    return pb.build()


def _air_plan(log, sh, rng):
    from test_air_program_cpu import denominators
    prog, e, n_cols = constraint_program(), log + 1, 7
    p = Plan(log=log, log_eval=e, program=prog, n_cols=n_cols)
    cols, start = m31(rng, n_cols, 1 << e), m31(rng, 4, 1 << e)
    pw, den = m31(rng, prog.n_constraints, 4), denominators(log, e)
    p.args.update(pw=pw, den=den)
    for k in range(n_cols):
        p.add(f"col{k}", cols[k], shift=sh.word())
    for q in range(4):           # the accumulator is added to (documented): 4 pointers, guarded one by one
        p.add(f"acc{q}", start[q], shift=sh.word())
    ref = O.eval_constraint_program(prog, list(cols), pw, den, log, e, acc4=list(start))
    for q in range(4):
        p.want(f"acc{q}", ref[q])
    return p


@entry("nx_eval_constraint_program", "air", "S", ("constraints.hip:57 NX_C_LOAD: gld(cols[a] + row)", "constraints.hip:88 NX_C_LOADE", "constraints.hip:112 the accumulator: words"), sizes=(2, 3, 5, 6),
       note="evaluation domain 2^(log + 1); the accumulator is added to")
def _eval_constraint_program(log, sh, rng, variant):
    return _air_plan(log, sh, rng)


@entry("nx_air_eval", "air", "S", ("air_jit.hip:305 generated loads G(cols[c])[row]: words", "air_jit.hip:319", "air_jit.hip:350 a0[r]", "air_jit.hip:50 G: a u32 pointer", "air_jit.hip:1599 the only 16-byte form is nx_trace_program's"), sizes=(2, 3, 5, 6),
       note="one recorded program, compiled once")
def _air_eval(log, sh, rng, variant):
    return _air_plan(log, sh, rng)


# ------------------------------------------------------------------------------------------------------------------ trace fills

@entry("nx_trace_prev_access", "fills", "B", ("access_history.cuh:532 vec = n >= 4 && aligned", "access_history.cuh:164 gld4_guarded", "access_history.cuh:170", "access_history.cuh:188 gst4 of all-idle quads", "access_history.cuh:189"),
       sizes=(1, 2, 3, 5, 6), vector_from="2^2 rows of a stream (one quad)")
def _prev_access(log, sh, rng, variant):
    import prev_access_model as M
    n, key_bits, n_payload = 1 << log, [3, 2], 2
    streams = []
    for s, lg in enumerate((log, max(log - 1, 1))):
        m = 1 << lg
        flag = rng.integers(0, 3, m, dtype=np.uint32)
        if m >= 8:
            flag[4:8] = 0          # an all-idle quad: the 16-byte zero stores
        streams.append({"key": [rng.integers(0, 8, m, dtype=np.uint32), rng.integers(0, 4, m, dtype=np.uint32)], "flag": flag if s == 0 else None,
                        "payload": [m31(rng, m), m31(rng, m)], "log_size": lg, "epoch": 0, "linear": False})
    ref = M.model(streams, key_bits, n_payload, init=[7, 9])
    p = Plan(log=log, key_bits=key_bits, n_payload=n_payload, init=[7, 9], n_streams=2, logs=[s["log_size"] for s in streams], has_flag=[True, False])
    for s, st in enumerate(streams):
        for k in range(2):
            p.add(f"s{s}key{k}", st["key"][k], shift=sh.word())
        if st["flag"] is not None:
            p.add(f"s{s}flag", st["flag"], shift=sh.word())
        for c in range(n_payload):
            p.add(f"s{s}pay{c}", st["payload"][c], shift=sh.word())
        for c in range(n_payload):
            p.add(f"s{s}prev{c}", words=1 << st["log_size"], shift=sh.word())
            p.want(f"s{s}prev{c}", ref["prev"][s][c])
        p.add(f"s{s}ord", words=1 << st["log_size"], shift=sh.word())
        p.want(f"s{s}ord", ref["ordinal"][s])
    p.host["n_keys"] = len(ref["keys"])
    return p


@entry("nx_trace_partition_fill", "fills", "S", ("trace_partition.hip:41 tp_load / tp_store: words", "trace_partition.hip:42", "trace_partition.hip:99", "trace_partition.hip:103"), sizes=(1, 3, 6), note="37 steps of 3 classes, a class destination and an NX_PART_ALL destination with is_pad and step")
def _partition_fill(log, sh, rng, variant):
    import trace_partition_model as M
    n_steps, n_classes = min(37, 1 << log), 3
    cls = rng.integers(0, n_classes, n_steps, dtype=np.uint32)
    cls[n_steps // 2] = M.NONE
    src = [rng.integers(0, 1 << 32, n_steps, dtype=np.uint64).astype(np.uint32) for _ in range(2)]
    counts, steps = M.partition(cls, n_classes)
    dests = [dict(cls=1, log_size=max(M.log_size(int(counts[1]), 1), 1), limbs=[(0, 0, 8), (0, 8, 8), (1, 0, 31)]),
             dict(cls=M.ALL, log_size=max(log, 1) if (1 << max(log, 1)) >= n_steps else log + 1, limbs=[(1, 16, 16), (0, 1, 31)])]
    p = Plan(log=log, n_steps=n_steps, n_classes=n_classes, dests=dests, counts=counts)
    p.add("class", cls, shift=sh.word())
    for k in range(2):
        p.add(f"src{k}", src[k], shift=sh.word())
    for d, dest in enumerate(dests):
        ref = M.fill(cls, n_classes, src, dest, steps)
        for k, col in enumerate(ref["cols"]):
            p.add(f"d{d}col{k}", words=1 << dest["log_size"], shift=sh.word())
            p.want(f"d{d}col{k}", col)
        p.add(f"d{d}pad", words=1 << dest["log_size"], shift=sh.word())
        p.want(f"d{d}pad", ref["is_pad"])
        p.add(f"d{d}step", words=1 << dest["log_size"], shift=sh.word())
        p.want(f"d{d}step", ref["step"])
    return p


def _keccak_columns(p, sh, prefix, cols):
    for k, c in enumerate(cols):           # every column its own pointer and its own guards
        p.add(f"{prefix}{k}", words=c.size, shift=sh.word())
        p.want(f"{prefix}{k}", c)


@entry("nx_trace_keccak_round", "fills", "W", ("keccak_store.h:14 a column word: *(u32*)(cols[col] + off)", "keccak_store.h:7 kr_gld64 of a state lane", "keccak_store.h:8 kr_gst64", "keccak_round.hip:68 refused on the host"),
       sizes=(3,), wide=[("d_states", 8, "keccak_store.h:7", None), ("d_states_out", 8, "keccak_store.h:8", None)],
       note="the header's own rule (8-byte lanes), refused before this work; the 1705 + 9 columns are written word by word and are shifted, each between guards")
def _keccak_round(log, sh, rng, variant):
    import keccak_round_model as R
    states = R.test_states(3, seed=1)
    ref = R.fill(states, 0, 1, log)
    p = Plan(log=log, n_instances=3, first_round=0, log_rounds=1, n_main=R.MAIN_COLS, n_pre=R.PRE_COLS)
    p.add("states", np.ascontiguousarray(states, "<u8").view(np.uint32), shift=sh.wide("d_states", 8))
    _keccak_columns(p, sh, "main", ref["main"])
    _keccak_columns(p, sh, "pre", ref["pre"])
    p.add("states_out", words=150, shift=sh.wide("d_states_out", 8))
    p.want("states_out", np.ascontiguousarray(ref["out"], "<u8").view(np.uint32))
    return p


@entry("nx_trace_keccak_memory_check", "fills", "W", ("keccak_store.h:14 a column word", "keccak_memcheck.hip:30 a 16-byte load of four timestamps", "keccak_memcheck.hip:45 an address: a word",
                                                      "keccak_store.h:7", "keccak_store.h:8", "keccak_memcheck.hip:85 refused on the host"),
       sizes=(3,), wide=[("d_states", 8, "keccak_store.h:7", None), ("d_timestamps", 16, "keccak_memcheck.hip:30", None), ("d_states_out", 8, "keccak_store.h:8", None)],
       note="the header's own rule, refused before this work; the 2001 + 1 columns and d_addresses are word accesses and are shifted")
def _keccak_memcheck(log, sh, rng, variant):
    import keccak_memcheck_model as K
    import keccak_round_model as R
    states = R.test_states(3, seed=2)
    addresses = np.array([4096, 0x1FFF0, 0xFFFFFF00], np.uint32)          # a 16-bit carry inside the 200 bytes, and one near the top
    ts = rng.integers(0, (1 << 32) - 1, (3, 200), dtype=np.uint64).astype(np.uint32)
    ts[0, 7] = 0xFFFF
    ref = K.fill(states, addresses, ts, log)
    p = Plan(log=log, n_instances=3, n_main=K.MAIN_COLS, n_pre=K.PRE_COLS)
    p.add("states", np.ascontiguousarray(states, "<u8").view(np.uint32), shift=sh.wide("d_states", 8))
    p.add("addresses", addresses, shift=sh.word())
    p.add("timestamps", ts, shift=sh.wide("d_timestamps", 16))
    _keccak_columns(p, sh, "main", ref["main"])
    _keccak_columns(p, sh, "pre", ref["pre"])
    p.add("states_out", words=150, shift=sh.wide("d_states_out", 8))
    p.want("states_out", np.ascontiguousarray(ref["out"], "<u8").view(np.uint32))
    return p


@entry("nx_trace_program", "fills", "B", ("air_jit.hip:1603 vec4 only when every touched column is 16-byte aligned", "air_jit.hip:1502 G4", "air_jit.hip:1541 GW4"), sizes=(1, 2, 3, 6),
       vector_from="2^2 rows, every load at offset 0 (context option trace.vec4)", note="tests/test_gpu_trace_program.py shifts one column; here every column, stores and a conditional store")
def _trace_program(log, sh, rng, variant):
    import nexus_zkvm_amd.air_program as ap
    import trace_programs as T
    pb = ap.ProgramBuilder()
    (x,), (f,) = pb.next_trace_mask(0), pb.next_trace_mask(1)
    pb.store(2, x * x + pb.row())                    # every word written: the column is FILL before the call
    pb.store_if(f, 3, pb.bxor(x, 5))                 # keeps its content where the flag is 0: in place
    prog = pb.build_trace_program()
    n = 1 << log
    nat = [rng.integers(0, 1 << 16, n).astype(np.uint64), (np.arange(n) % 2).astype(np.uint64), np.zeros(n, np.uint64), np.full(n, T.SENTINEL, np.uint64)]
    ref = T.interp(prog, nat, log)
    p = Plan(log=log, program=prog, n_cols=4)
    for k in (0, 1):
        p.add(f"col{k}", T.to_storage(nat[k]), shift=sh.word())
    p.add("col2", words=n, shift=sh.word())
    p.add("col3", T.to_storage(nat[3]), shift=sh.word())
    p.want("col2", T.to_storage(ref[2]))
    p.want("col3", T.to_storage(ref[3]))
    return p


# ------------------------------------------------------------------------------------------------------------------ the session's slabs

SESSION_LOGS = (1, 1, 1, 2, 2, 5)      # runs of 3, 2 and 1 columns: nx_prover_tree_begin packs each run into one slab


def session_case(mode):
    """(log sizes, host columns, the oracle session's root of their commit) for the hash mode; the oracle accepts columns of 2 rows"""
    rng = np.random.default_rng(77 + mode)
    host = [edge(m31(rng, 1, 1 << l))[0] for l in SESSION_LOGS]
    root = O.ProverSession(O.default_cfg(hash_mode=mode), max(SESSION_LOGS) + 1, threads=1).commit([h.copy() for h in host])
    _, root2 = O.lde_commit([h.copy() for h in host], 1, mode, threads=1)
    assert np.array_equal(root, root2)      # the oracle's two routes agree
    return list(SESSION_LOGS), host, root


# ------------------------------------------------------------------------------------------------------------------ the case list

VARIANTS = {
    "nx_merkle_commit": ("", "mixed", "raw0", "mixed-raw0"),
    "nx_merkle_commit_on_layer": ("", "leaf", "nodes-raw0"),
    "nx_merkle_leaf_chain": ("", "raw0"),
    "nx_merkle_from_leaves": ("", "raw0"),
    "nx_batch_inverse_m31": ("", "alias"),
    "nx_batch_inverse_qm31": ("", "alias"),
    "nx_logup_finalize_col": ("", "alias"),
    "nx_logup_col": ("", "alias"),
    "nx_logup_cols_batched": ("", "explicit"),
    "nx_upload_columns": ("coset", "circle"),
    "nx_upload_columns_narrow": ("coset", "circle"),
}


# W entries that also take columns their kernels touch word by word (those are shifted), or whose wide access is 8 bytes (2 words is legal)
W_WITH_WORD_ARGS = ("nx_merkle_commit_on_layer", "nx_merkle_leaf_chain", "nx_fold_circle_into_line", "nx_fold_line", "nx_m31_widen", "nx_m31_narrow",
                    "nx_trace_keccak_round", "nx_trace_keccak_memory_check")


def _refusal_shifts(nbytes):
    return (1, 2, 3) if nbytes == 16 else (1, 3)


def cases():
    out = []
    for name, row in TABLE.items():
        for variant in VARIANTS.get(name, ("",)):
            for log in row.sizes:
                if name == "nx_merkle_commit" and log == FUSED_LOG and "mixed" in variant:
                    continue
                for s in SHIFTS:
                    if s and row.cls == "W" and name not in W_WITH_WORD_ARGS and not (row.exempt_below is not None and log < row.exempt_below):
                        continue          # every argument is wide: the only placement the contract allows is shift 0
                    out.append(Case(name, log, s, variant, None))
        if row.cls == "W":        # the refusal: at the first size that is not exempt, every forbidden offset of every wide argument
            log = min(l for l in row.sizes if row.exempt_below is None or l >= row.exempt_below)
            for w in row.wide:
                for s in _refusal_shifts(w.bytes):
                    out.append(Case(name, log, 0, VARIANTS.get(name, ("",))[0], (w.arg, s, w.index)))
    return out


CASES = cases()
FAMILIES = ("transforms", "merkle", "pcs", "field", "layout", "logup", "air", "fills")


def family_cases(family):
    return [c for c in CASES if TABLE[c.entry].family == family]
