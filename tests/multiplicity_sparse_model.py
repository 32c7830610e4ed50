"""nx_logup_multiplicities_sparse in numpy: the model the device call and the host emulation are compared with.

The table is a sparse subset of a key space of up to 32 bits, so nothing here is sized by the key space: the valid table keys are
sorted (np.unique), a looked-up key finds its table row with np.searchsorted, the weighted sums are exact Python integers reduced mod
p once.  The missing rule and the two table refusals are those of include/nexus_hip.h."""
import numpy as np

P = (1 << 31) - 1


def split(keys, key_bits):
    """packed keys -> one uint32 column per key column"""
    out, shift = [], 0
    for b in key_bits:
        out.append(((np.asarray(keys, np.uint64) >> np.uint64(shift)) & np.uint64((1 << b) - 1)).astype(np.uint32))
        shift += b
    return out


def pack(cols, key_bits):
    """(packed keys as uint64, mask of the rows with every entry inside its bits) of rows given as one column per key column"""
    assert 1 <= len(key_bits) <= 4 and len(cols) == len(key_bits) and all(1 <= b <= 32 for b in key_bits) and sum(key_bits) <= 32
    key, ok, shift = np.zeros(len(cols[0]), np.uint64), np.ones(len(cols[0]), bool), 0
    for c, b in zip(cols, key_bits):
        c = np.asarray(c, np.uint64)
        ok &= c < np.uint64(1 << b)
        key |= (c & np.uint64((1 << b) - 1)) << np.uint64(shift)
        shift += b
    return key, ok


class TableRefused(Exception):
    """NX_ERR_ARG of the table: kind "range" (pos) or "duplicate" (first, second, entries)"""

    def __init__(self, kind, **kw):
        super().__init__(kind, kw)
        self.kind = kind
        self.__dict__.update(kw)


def index(table, valid, key_bits):
    """The sorted valid keys and, for each, the position of its table row.  Raises TableRefused as the device call refuses."""
    n = len(table[0])
    is_row = np.ones(n, bool) if valid is None else np.asarray(valid) != 0
    pos = np.nonzero(is_row)[0]
    key, ok = pack([np.asarray(c)[pos] for c in table], key_bits)
    if not ok.all():
        raise TableRefused("range", pos=int(pos[~ok].min()))
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    if len(uniq) != len(key):
        later = np.ones(len(key), bool)
        later[first] = False                  # np.unique names the first occurrence: positions ascend
        second = int(np.nonzero(later)[0].min())
        raise TableRefused("duplicate", first=int(pos[first[inverse[second]]]), second=int(pos[second]),
                           entries=tuple(int(np.asarray(c)[pos[second]]) for c in table))
    return uniq, pos[first]


def multiplicities(uses, table, valid, key_bits):
    """uses: (columns, weights or None) of host arrays; table: columns; valid: None or a column.
    -> (mult column of the table's length, sorted (use, position) of the missing rows)"""
    uniq, where = index(table, valid, key_bits)
    sums = [0] * len(uniq)                    # Python integers: exact whatever the weights
    missing = []
    for u, (cols, w) in enumerate(uses):
        key, ok = pack(cols, key_bits)
        w = np.ones(len(key), np.uint64) if w is None else np.asarray(w, np.uint64)
        at = np.searchsorted(uniq, key)
        found = np.zeros(len(key), bool)
        inside = at < len(uniq)
        found[inside] = uniq[at[inside]] == key[inside]
        live = w != 0
        good = live & ok & found
        for i, x in zip(at[good].tolist(), w[good].tolist()):
            sums[i] += x
        missing += [(u, int(p)) for p in np.nonzero(live & ~(ok & found))[0]]
    mult = np.zeros(len(table[0]), np.uint32)
    mult[where] = np.array([s % P for s in sums], np.uint32) if len(sums) else np.zeros(0, np.uint32)
    return mult, sorted(missing)
