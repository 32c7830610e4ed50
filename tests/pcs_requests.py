"""The request structures of tests/test_pcs_requests_cpu.py and tests/test_gpu_pcs_requests.py: plain data and small helpers.

The per-op calls of include/nexus_hip.h (INTEGRATION.md maps them onto the trait methods of a per-op HipBackend) take a REQUEST: how
many batches, points, queries or nonces, and how they are grouped, ordered, repeated or split across launches.  The whole-prove entries
only ever build a handful of such shapes; the lists below sweep that axis for nx_accumulate_quotients, nx_accumulate_quotients_partial,
nx_eval_at_points, nx_grind, nx_gather and nx_merkle_decommit.

Conditions of every case, not under test here: sample points and alphas are drawn from the oracle's channel (as _random_point_and_alpha
of tests/test_gpu_parity.py does), so every sample point lies off the domain and every quotient denominator is non-zero (the CPU file
checks that for the listed points); columns are uniform random below P from fixed seeds, never constant, so that an index mistake shows.

The second half of the module is a plain-integer restatement of the row formula documented in oracle/pcs.h (quotient_constants and
accumulate_row_quotients): Python ints mod P, CM31 and QM31 as tuples, no oracle.  The oracle is "PARITY UNPINNED"; empty batches,
repeated columns and split entries are where nothing else cross-checks it."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

P = (1 << 31) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOT_LOCAL = 0xFFFFFFFF                       # col_idx of an entry whose column another rank holds: ignored by the library


def channel_points(oracle, seed, n_points):
    """n_points sample points (8 words, x then y) and one alpha (4 words) from the oracle's channel after mix_u64(seed)."""
    L = oracle.lib()
    ch = C.c_void_p(L.orc_channel_new())
    L.orc_channel_mix_u64(ch, seed)
    pts = [np.zeros(8, np.uint32) for _ in range(n_points)]
    for p in pts:
        L.orc_get_random_point(ch, oracle.ptr(p))
    alpha = np.zeros(4, np.uint32)
    L.orc_channel_draw_secure_felt(ch, oracle.ptr(alpha))
    L.orc_channel_free(ch)
    return pts, alpha


def rand_cols(seed, n_cols, log):
    return np.random.default_rng(seed).integers(0, P, (n_cols, 1 << log), dtype=np.uint32)


# ---- 1. quotient requests -----------------------------------------------------------------------------------------------------------
QUOT_LOGS = (1, 2, 5, 11)                    # quotient_small_kernel; one lane; 8 lanes; 512 lanes = two blocks of quotient_kernel
N_COLS = 9
FULL = tuple(range(N_COLS))
PERMUTED = (5, 2, 8, 0, 7, 3, 1, 6, 4)
# name -> [(index of the sample point, column indices in entry order), ...]
STRUCTURES = {
    "S0": [],                                                                    # n_batches == 0: the output is all zero
    "S1": [(0, (4,))],                                                           # one batch of one entry
    "S2": [(0, FULL), (1, ()), (2, FULL)],                                       # an empty batch between two full ones
    "S3": [(0, ()), (1, FULL)],                                                  # the first batch empty
    "S4": [(0, FULL), (1, ())],                                                  # the last batch empty
    "S5": [(0, (3, 3, 3, 3))],                                                   # column 3 four times (four values), column 0 never
    "S6": [(0, PERMUTED)],                                                       # every column, in a non-monotone order
    "S7": [(0, (0, 2, 4, 6, 8)), (0, (1, 3, 5, 7, 2))],                          # one point carried by two batches
    "S8": [(b, tuple((2 * b + j) % N_COLS for j in range(b + 1))) for b in range(9)],   # counts 1 .. 9: every residue of the 4-wide loop
    "S9": [(b, (6,)) for b in range(5)],                                         # every batch holds the same single column
}
N_POINTS = 9


def quotient_request(oracle, log, name):
    """(columns [N_COLS, 2^log], alpha, batches) of structure `name` at `log`; batches = [(point8, [(col, value4), ...]), ...], the
    form HipBackend.accumulate_quotients takes.  Points and alpha depend on the log only, values on the log and the structure."""
    pts, alpha = channel_points(oracle, 700 + log, N_POINTS)
    rng = np.random.default_rng([log, int(name[1:]), 71])
    batches = [(pts[p], [(c, rng.integers(0, P, 4, dtype=np.uint32)) for c in cols]) for p, cols in STRUCTURES[name]]
    return rand_cols(7100 + log, N_COLS, log), alpha, batches


def flatten(batches):
    """The flattened arrays of the C ABI: points (8 per batch), counts, column indices, values (4 per entry).  Never zero-sized."""
    n = sum(len(b[1]) for b in batches)
    pts, counts = np.zeros(8 * max(1, len(batches)), np.uint32), np.zeros(max(1, len(batches)), np.uint32)
    cidx, vals = np.zeros(max(1, n), np.uint32), np.zeros(4 * max(1, n), np.uint32)
    k = 0
    for b, (pt, entries) in enumerate(batches):
        pts[8 * b:8 * b + 8] = pt
        counts[b] = len(entries)
        for c, v in entries:
            cidx[k] = c
            vals[4 * k:4 * k + 4] = v
            k += 1
    return pts, counts, cidx, vals


def oracle_quotients(oracle, log, cols, alpha, batches):
    pts, counts, cidx, vals = flatten(batches)
    outs = [np.zeros(1 << log, np.uint32) for _ in range(4)]
    host = [np.ascontiguousarray(c) for c in cols]
    oracle.lib().orc_accumulate_quotients(log, oracle.ptr_array(host), len(host), oracle.ptr(alpha), len(batches), oracle.ptr(pts),
                                          oracle.ptr(counts.astype(np.int32)), oracle.ptr(cidx.astype(np.int32)), oracle.ptr(vals), 2,
                                          oracle.ptr_array(outs))
    return np.stack(outs)


# ---- 2. partial quotients: the statement split over the ranks of a column-sharded prove ------------------------------------------
PARTIAL_STATEMENTS = ("S2", "S5", "S6", "S8")
PARTIAL_LOGS = (1, 2, 11)
WORLDS = (2, 3)
SPLITS = ("round-robin", "blocks", "rank0-empty")


def column_owner(split, world):
    """owner[c] = the rank that holds column c."""
    if split == "round-robin":
        return [c % world for c in range(N_COLS)]
    if split == "blocks":
        return [c * world // N_COLS for c in range(N_COLS)]
    return [1 + c % (world - 1) for c in range(N_COLS)]            # rank 0 owns nothing: it calls with n_cols == 0


def rank_request(batches, owner, rank):
    """What `rank` passes: (its columns' global indices in its local order, the batches with col_idx renumbered to that order for its
    own entries and NOT_LOCAL for the others, entry_local: one flag per flattened entry)."""
    mine = [c for c in range(N_COLS) if owner[c] == rank]
    renumbered = [(pt, [(mine.index(c) if owner[c] == rank else NOT_LOCAL, v) for c, v in entries]) for pt, entries in batches]
    local = [int(owner[c] == rank) for _, entries in batches for c, _ in entries]
    return mine, renumbered, np.array(local, np.uint8)


# ---- 3. evaluation requests -----------------------------------------------------------------------------------------------------------
EVAL_LOGS = (0, 3, 10, 11)                   # a lone coefficient; below the low table; n_hi = 1; n_hi = 2
EVAL_POLYS = 4
EVAL_POINTS = 3
INTERLEAVED = dict(points=(0, 1, 0, 2, 1, 0, 2), poly_idx=(3, 3, 0, 1, 3, 2, 0))     # p1 p2 p1 p3 p2 p1 p3
REPEATED = dict(points=(0, 1, 0, 0), poly_idx=(2, 2, 2, 1))                           # (polynomial 2, p1) asked twice
SLAB = 32768                                 # polynomials of one point per launch of eval_at_point_kernel (csrc/pcs.hip)
SLAB_LOG = 3


def eval_request(oracle, log):
    """(coefficient columns [EVAL_POLYS, 2^log], the EVAL_POINTS sample points) of `log`."""
    pts, _ = channel_points(oracle, 800 + log, EVAL_POINTS)
    return rand_cols(8100 + log, EVAL_POLYS, log), pts


def slab_case():
    """(point index, poly_idx) per evaluation: point 0 carries SLAB + 5 evaluations, poly_idx = j % 4 over its j-th evaluation and
    (j + 1) % 4 from the slab boundary on; point 1 carries 3, at positions 0, 16384 and the last — so it is the FIRST group."""
    n = SLAB + 5 + 3
    sel = np.zeros(n, np.int64)
    sel[[0, 16384, n - 1]] = 1
    poly = np.zeros(n, np.uint32)
    j = np.arange(SLAB + 5)
    poly[sel == 0] = np.where(j < SLAB, j % 4, (j + 1) % 4)
    poly[sel == 1] = (0, 2, 3)
    return sel, poly


def oracle_evals(oracle, polys, pts, sel, poly_idx):
    """out[i] = polys[poly_idx[i]](pts[sel[i]]): the oracle once per distinct (polynomial, point), broadcast."""
    sel, poly_idx = np.asarray(sel, np.int64), np.asarray(poly_idx, np.int64)
    table = np.zeros((len(pts), len(polys), 4), np.uint32)
    for s, p in sorted({(int(s), int(p)) for s, p in zip(sel, poly_idx)}):
        table[s, p] = oracle.eval_at_point(polys[p], pts[s])
    return table[sel, poly_idx]


# ---- 4. grind beyond the first launch --------------------------------------------------------------------------------------------------
GRIND_BITS = 24
GRIND_FILE = os.path.join(GOLDEN, "grind_launches.json")      # (seed, digest words, smallest nonce), recorded from the oracle
GRIND_LAUNCHES = {2: 1, 1: 2, 10: 3}                          # seed -> the launch of nx_grind that finds its nonce


def grind_cases():
    with open(GRIND_FILE) as f:
        doc = json.load(f)
    assert doc["pow_bits"] == GRIND_BITS
    return {c["seed"]: (np.array(c["digest"], np.uint32), int(c["nonce"])) for c in doc["cases"]}


def grind_windows(bits, n):
    """[lo, hi) of the first n launches of nx_grind (csrc/merkle.hip), restated: the first batch is min(2^24, max(2^16, 64 << min(bits,
    18))) nonces, each later one twice the one before, capped at 2^24."""
    batch = min(1 << 24, max(1 << 16, 64 << min(bits, 18)))
    base, out = 0, []
    for _ in range(n):
        out.append((base, base + batch))
        base += batch
        batch = min(1 << 24, 2 * batch)
    return out


def pow_zero_bits(digest_words, nonce):
    """Trailing zero bits of Blake2s(digest ‖ nonce_le64), its first 16 bytes read as a little-endian integer."""
    h = hashlib.blake2s(np.asarray(digest_words, np.uint32).tobytes() + int(nonce).to_bytes(8, "little")).digest()
    v = int.from_bytes(h[:16], "little")
    return 128 if v == 0 else (v & -v).bit_length() - 1


# ---- 5. gather ----------------------------------------------------------------------------------------------------------------------
GATHER_LOGS = (10, 4, 10)
BIG_LOG = 28                                 # one column of 2^28 words = 1 GiB: byte offsets up to 2^30 - 4


# ---- 6. decommit requests ---------------------------------------------------------------------------------------------------------------
DECOMMIT_LOGS = [9] * 5 + [7] * 3 + [9] * 2 + [4]              # the mixed tree of test_merkle_decommit_matches_oracle
DECOMMIT_QUERIES = {
    "sibling-pairs": {9: [6, 7, 300, 301]},                    # both children queried: no hash witness for the pair
    "whole-layer": {4: list(range(16)), 9: [0]},
    "one-query": {9: [511]},
    "layer-without-column": {8: [5, 200], 9: [10]},
    "small-layer-only": {4: [0, 15]},                          # the 2^9 and 2^7 columns are never queried
    "first-and-last": {9: [0, 511], 7: [0, 127], 4: [0, 15]},
}


def decommit_columns():
    return [np.random.default_rng(900 + i).integers(0, P, 1 << l, dtype=np.uint32) for i, l in enumerate(DECOMMIT_LOGS)]


def oracle_decommit(oracle, host, mode, queries):
    """(queried values, hash witness [n, 8], column witness) of the oracle; the buffers are sized by a first, output-less call."""
    logs = np.array(DECOMMIT_LOGS, np.int32)
    qlogs = np.array(sorted(queries), np.int32)
    qcnt = np.array([len(queries[int(l)]) for l in qlogs], np.int32)
    qs = np.array([q for l in qlogs for q in queries[int(l)]], np.uint64)
    n_out = (C.c_size_t * 3)()
    args = (oracle.ptr_array(host), oracle.ptr(logs), len(host), mode, oracle.ptr(qlogs), oracle.ptr(qcnt), len(qlogs), oracle.ptr(qs))
    oracle.lib().orc_merkle_decommit(*args, None, None, None, n_out)
    qv, hw, cw = np.zeros(max(1, n_out[0]), np.uint32), np.zeros(max(1, 8 * n_out[1]), np.uint32), np.zeros(max(1, n_out[2]), np.uint32)
    sizes = tuple(n_out)
    oracle.lib().orc_merkle_decommit(*args, oracle.ptr(qv), oracle.ptr(hw), oracle.ptr(cw), n_out)
    assert tuple(n_out) == sizes
    return qv[:sizes[0]], hw[:8 * sizes[1]].reshape(-1, 8), cw[:sizes[2]]


# ---- the row formula of oracle/pcs.h in plain integers ------------------------------------------------------------------------------
# M31: ints mod P.  CM31 = (a, b) = a + b i, i^2 = -1.  QM31 = (A, B) = A + B u with A, B in CM31, u^2 = 2 + i; its four words are
# (A.a, A.b, B.a, B.b).
C_ZERO, Q_ZERO, Q_ONE, R = (0, 0), ((0, 0), (0, 0)), ((1, 0), (0, 0)), (2, 1)


def c_add(x, y): return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)
def c_sub(x, y): return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)
def c_neg(x): return (-x[0] % P, -x[1] % P)
def c_mul(x, y): return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def c_inv(x):
    d = pow((x[0] * x[0] + x[1] * x[1]) % P, P - 2, P)
    return (x[0] * d % P, -x[1] * d % P)


def q_add(x, y): return (c_add(x[0], y[0]), c_add(x[1], y[1]))
def q_sub(x, y): return (c_sub(x[0], y[0]), c_sub(x[1], y[1]))
def q_mul(x, y): return (c_add(c_mul(x[0], y[0]), c_mul(R, c_mul(x[1], y[1]))), c_add(c_mul(x[0], y[1]), c_mul(x[1], y[0])))
def q_mul_c(x, c): return (c_mul(x[0], c), c_mul(x[1], c))
def q_mul_m(x, s): return q_mul_c(x, (s % P, 0))
def q_conj(x): return (x[0], c_neg(x[1]))                      # the conjugate over CM31: u -> -u
def q_from_words(w): return ((int(w[0]), int(w[1])), (int(w[2]), int(w[3])))
def q_words(x): return [x[0][0], x[0][1], x[1][0], x[1][1]]


GEN = (2, 1268011823)                        # the generator of the circle group of order 2^31


def pt_add(p, q): return ((p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P)


def pt_from_index(idx):
    res, cur, idx = (1, 0), GEN, idx % (1 << 31)
    while idx:
        if idx & 1:
            res = pt_add(res, cur)
        cur, idx = pt_add(cur, cur), idx >> 1
    return res


def domain_point(log, row):
    """The point of CanonicCoset(log).circle_domain() behind bit-reversed row `row`: the half coset half_odds(log - 1) — initial index
    2^(31 - (log + 1)), step 2^(31 - (log - 1)) — and then its conjugate."""
    i = int(format(row, "0%db" % log)[::-1], 2)
    half = 1 << (log - 1)
    at = lambda j: (1 << (30 - log)) + (1 << (32 - log)) * j
    return pt_from_index(at(i) if i < half else -at(i - half))


def denominator(log, row, pt):
    """(Re p.x - d.x) Im p.y - (Re p.y - d.y) Im p.x in CM31, Re / Im the CM31 halves of a QM31 coordinate."""
    px, py, (dx, dy) = q_from_words(pt[:4]), q_from_words(pt[4:]), domain_point(log, row)
    return c_sub(c_mul(c_sub(px[0], (dx, 0)), py[1]), c_mul(c_sub(py[0], (dy, 0)), px[1]))


def model_quotients(log, cols, alpha, batches, local=None, include_line=True):
    """accumulate_row_quotients over every row.  Per batch, entry k (1-based) has alpha^k and the line through (p.y, v), (conj p.y,
    conj v): a = conj v - v, c = conj p.y - p.y, b = v c - a p.y; the row's numerator is Σ_k alpha^k (c f_k(d) - (a d.y + b)), the
    accumulator acc <- acc alpha^count + numerator / denominator.  `local` (one flag per flattened entry, None = all) keeps the column
    term of the flagged entries only, `include_line` the -(a d.y + b) terms of ALL entries: what one rank of a column-sharded prove
    computes.  Returns 2^log rows of 4 words."""
    alpha = q_from_words(alpha)
    consts, k = [], 0
    for pt, entries in batches:
        py = q_from_words(pt[4:])
        c = q_sub(q_conj(py), py)
        a_pow, lines = Q_ONE, []
        for col, v in entries:
            a_pow = q_mul(a_pow, alpha)
            v = q_from_words(v)
            a = q_sub(q_conj(v), v)
            b = q_sub(q_mul(v, c), q_mul(a, py))
            lines.append((col, q_mul(a_pow, a), q_mul(a_pow, b), q_mul(a_pow, c), local is None or bool(local[k])))
            k += 1
        consts.append((pt, lines, a_pow))
    out = []
    for r in range(1 << log):
        dy = domain_point(log, r)[1]
        acc = Q_ZERO
        for pt, lines, coeff in consts:
            num = Q_ZERO
            for col, la, lb, lc, is_local in lines:
                if is_local:
                    num = q_add(num, q_mul_m(lc, int(cols[col][r])))
                if include_line:
                    num = q_sub(num, q_add(q_mul_m(la, dy), lb))
            acc = q_add(q_mul(acc, coeff), q_mul_c(num, c_inv(denominator(log, r, pt))))
        out.append(q_words(acc))
    return out
