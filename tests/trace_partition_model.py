"""The judge of nx_trace_partition_create / nx_trace_partition_fill, stated without a look at the kernels: a stable argsort of the class
column gives every class its steps in execution order; a storage position holds the natural row that the circle domain puts there
(position = bit reversal of the domain index; the domain holds the even coset rows in its first half and the odd ones, backwards, in
its second); a limb is cut from a Python integer.  Used by tests/test_trace_partition_cpu.py and tests/test_gpu_trace_partition.py; all
comparisons against it are exact word equalities."""
import numpy as np

P = (1 << 31) - 1
NONE = ALL = 0xFFFFFFFF


def coset_row_of_pos(pos, log):
    d = int(format(pos, "0%db" % log)[::-1], 2) if log else 0
    n = 1 << log
    return 2 * d if d < n // 2 else 2 * (n - 1 - d) + 1


_ROWS = {}


def rows_of_positions(log):
    """natural row of every storage position of a 2^log-row column: coset_row_of_pos at every position, bit by bit over an array
    (pinned against the scalar definition by the CPU test), kept per size"""
    if log not in _ROWS:
        pos, d, n = np.arange(1 << log, dtype=np.int64), np.zeros(1 << log, np.int64), 1 << log
        for b in range(log):
            d |= ((pos >> b) & 1) << (log - 1 - b)
        _ROWS[log] = np.where(d < n // 2, 2 * d, 2 * (n - 1 - d) + 1)
    return _ROWS[log]


def log_size(count, min_log):
    """max(ceil_log2(count), min_log); count 0 gives min_log"""
    log = 0
    while (1 << log) < count:
        log += 1
    return max(log, min_log)


def limb(word, shift, bits):
    v = (int(word) >> shift) & ((1 << bits) - 1)
    return 0 if v == P else v


def first_bad(cls, n_classes):
    """the smallest step whose class word is neither a class nor NONE, or None"""
    for j, w in enumerate(np.asarray(cls, np.uint32).tolist()):
        if w >= n_classes and w != NONE:
            return j, w
    return None


def partition(cls, n_classes):
    """(counts, steps): steps[c] = the steps of class c in execution order, from ONE stable argsort of the class column"""
    cls = np.asarray(cls, np.uint32)
    order = np.argsort(cls, kind="stable")
    sorted_cls = cls[order]
    steps = [order[np.searchsorted(sorted_cls, c, "left"):np.searchsorted(sorted_cls, c, "right")].astype(np.int64) for c in range(n_classes)]
    return np.array([len(s) for s in steps], np.uint32), steps


def limbs_of(words, shift, bits):
    """limb() over an array: 64-bit integers, so that no shift or mask can wrap (pinned against limb() by the CPU test)"""
    v = (np.asarray(words, np.uint32).astype(np.uint64) >> np.uint64(shift)) & np.uint64((1 << bits) - 1)
    v[v == P] = 0
    return v.astype(np.uint32)


def fill(cls, n_classes, src, dest, steps_of=None):
    """dest: dict with cls, log_size, limbs [(src, shift, bits)].  -> {"cols": [column per limb], "is_pad", "step"} as uint32 arrays in
    storage order.  steps_of: partition(cls, n_classes)[1] when the caller has it already."""
    n = len(cls)
    steps = np.arange(n, dtype=np.int64) if dest["cls"] == ALL else (steps_of or partition(cls, n_classes)[1])[dest["cls"]]
    log = dest["log_size"]
    assert len(steps) <= (1 << log)
    rows = rows_of_positions(log)
    real = rows < len(steps)
    step = np.zeros(1 << log, np.int64)
    step[real] = steps[rows[real]]
    cols = []
    for s, shift, bits in dest["limbs"]:
        col = np.zeros(1 << log, np.uint32)
        col[real] = limbs_of(np.asarray(src[s], np.uint32)[step[real]], shift, bits)
        cols.append(col)
    return {"cols": cols, "is_pad": (~real).astype(np.uint32), "step": step.astype(np.uint32)}


def to_storage(natural, log):
    """a column given in natural row order -> storage order"""
    return np.asarray(natural)[rows_of_positions(log)]
