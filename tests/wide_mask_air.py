"""A recorded AIR whose masks reach further than the neighbour row, with valid traces: the statement of tests/test_wide_masks_cpu.py
and tests/test_gpu_wide_masks.py.  Plain data and small helpers, in the manner of tests/air_examples.py and tests/size_lattice.py.

The C ABI lets a recorded AIR read a column at any int32 row offset (NX_C_LOAD / NX_C_LOADE, nx_air_component.mask_offsets); the other
statements of the suite stay inside {-1, 0, +1}.  The window component reads one base-field column `a` at four offsets b0 .. b3 and one
secure column `T` at two offsets s0, s1:

    main columns (16):  a | w | h3 | h4 | T (4 coordinates) | U (4) | V (4)
    w  = a@b0 * a@b3 + a@b1 + 5 * a@b2          degree 2
    h3 = a@b0 * a@b3 * a@b2                     degree 3
    h4 = h3 * a@b1                              degree 4
    U  = T@s0 * T@s1                            degree 2, secure
    V  = U * a@b2                               degree 3, secure

x@o is row (i + o) mod N of the natural trace order: offsets reduce modulo the trace length, whatever their size.  Two entries of one
mask that coincide modulo N are two samples at the same point (COINCIDE below)."""
import numpy as np

import oracle_lib as O

P = O.P
N_MAIN = 16
COL_A, COL_W, COL_H3, COL_H4, COL_T, COL_U, COL_V = 0, 1, 2, 3, 4, 8, 12

# ---- the offset sets: (base offsets b0 .. b3 of `a`, secure offsets s0, s1 of `T`) ------------------------------------------------
STD = ((-2, -1, 1, 3), (-3, 2))
COINCIDE = ((-1, 3, 4, 0), (0, 4))             # on a 4-row trace: -1 = 3 and 4 = 0, so two mask entries share one point, twice
HUGE = ((-(2 ** 31), 2 ** 31 - 1, 2 ** 20 + 1, -2 ** 20 - 3), (2 ** 30, -2 ** 30 - 1))     # both ends of int32: the same wrap as everything else
WIDE = ((-2, 3, -2, 3), (0, 0))                # wide_variant: a at -2 and +3 only, T at 0: three sample points in all


def FAR(N):
    """Offsets of N and more on an N-row trace: every one wraps at least once."""
    return ((-N - 1, N - 1, N, 2 * N + 1), (-N, N + 3))


def offsets_of(name, log):
    return {"STD": STD, "COINCIDE": COINCIDE, "HUGE": HUGE, "WIDE": WIDE}[name] if name != "FAR" else FAR(1 << log)


SIZES = (2, 3, 4, 5, 7)                        # half- and quarter-domain need log_size >= 4: 3 and 4 straddle that line; 2 is where offsets coincide

# ---- the cases: (logs, offset set).  The CPU file proves every one on the oracle; the GPU file proves them on the device. -----------
SESSION_CASES = [((2,), "STD"), ((3,), "STD"), ((4,), "STD"), ((5, 2), "STD"), ((3, 4, 5), "STD"), ((7, 4), "STD"),
                 ((3,), "FAR"), ((4,), "FAR"), ((2,), "COINCIDE"), ((5,), "HUGE")]
# name -> (oracle_lib.default_cfg keywords, high_degree)
CONFIGS = {
    "b1-lcd1": (dict(pow_bits=2, log_blowup=1, log_constraint_degree=1), False),
    "b1-lcd2": (dict(pow_bits=2, log_blowup=1, log_constraint_degree=2), True),
    "b2-lcd2": (dict(pow_bits=2, log_blowup=2, log_constraint_degree=2), True),
}
BOUNDS_CASE = ((7, 4), "STD", (2, 1))          # per-component bounds under b1-lcd2
SHARDED_CASES = [((9,), "STD"), ((7, 4), "STD")]
CONTROL_CASE = ((5,), "STD")
WIDE_LOGS = (5, 9)
PAD = 128                                      # free columns of wide_variant: 1 preprocessed + 16 + 128 columns of one size, 3 points
COEFFS_COLUMNS_PER_POINT = 48                  # csrc/prover.hip: the coefficient quotients are taken when columns >= 48 * points


# ---- vectorised field arithmetic (uint64 arrays of canonical words) --------------------------------------------------------------
def _cmul(a, b):
    return ((a[0] * b[0] + (P - (a[1] * b[1]) % P)) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def qmul_rows(x, y):
    """QM31 = CM31[u] / (u^2 - 2 - i), CM31 = M31[i] / (i^2 + 1): x, y lists of 4 uint64 arrays; pinned against orc_qm31_mul by the CPU file."""
    aa, bb = _cmul(x[:2], y[:2]), _cmul(x[2:], y[2:])
    ab, ba = _cmul(x[:2], y[2:]), _cmul(x[2:], y[:2])
    r0, r1 = (2 * bb[0] + P - bb[1]) % P, (2 * bb[1] + bb[0]) % P
    return [(aa[0] + r0) % P, (aa[1] + r1) % P, (ab[0] + ba[0]) % P, (ab[1] + ba[1]) % P]


def at(x, o):
    """x@o: row (i + o) mod N of a natural-order column"""
    n = len(x)
    return x[(np.arange(n, dtype=np.int64) + int(o)) % n]


# ---- the trace ---------------------------------------------------------------------------------------------------------------------
def window_trace(log, seed, base, sec, pad=0):
    """The 16 main columns (+ `pad` free ones) of a valid window trace: (natural order, finalized to bit-reversed circle-domain order)."""
    rng = np.random.default_rng(seed)
    n = 1 << log
    a = rng.integers(0, P, n, dtype=np.uint64)
    T = [rng.integers(0, P, n, dtype=np.uint64) for _ in range(4)]
    b0, b1, b2, b3 = (at(a, o) for o in base)
    w = (b0 * b3 % P + b1 + 5 * b2) % P
    h3 = b0 * b3 % P * b2 % P
    h4 = h3 * b1 % P
    U = qmul_rows([at(t, sec[0]) for t in T], [at(t, sec[1]) for t in T])
    V = [u * b2 % P for u in U]
    free = [rng.integers(0, P, n, dtype=np.uint64) for _ in range(pad)]
    nat = [x.astype(np.uint32) for x in [a, w, h3, h4] + T + U + V + free]
    return nat, [O.finalize_column(x) for x in nat]


def window_component(ap, log, main0, base, sec, bound=0, high_degree=False, pad=0):
    """The recorded component over main columns main0 .. main0 + 15 (+ pad) of tree 1.  Constraints, in order: with high_degree
    h4 - a0 a3 a2 a1 (degree 4); w - a0 a3 - a1 - 5 a2; with high_degree h3 - a0 a3 a2 (degree 3); u - t0 t1 (secure); with high_degree
    v - t0 t1 a2 (secure, degree 3).  nx_air_constraint_degrees: [4, 2, 3, 2, 3], or [2, 2]."""
    pb = ap.ProgramBuilder()
    a0, a1, a2, a3 = pb.next_trace_mask(COL_A, base)
    (w,) = pb.next_trace_mask(COL_W)
    (h3,) = pb.next_trace_mask(COL_H3)
    (h4,) = pb.next_trace_mask(COL_H4)
    t0, t1 = pb.next_secure_mask(COL_T, sec)
    (u,) = pb.next_secure_mask(COL_U)
    (v,) = pb.next_secure_mask(COL_V)
    if high_degree:
        pb.add_constraint(h4 - a0 * a3 * a2 * a1)
    pb.add_constraint(w - a0 * a3 - a1 - 5 * a2)
    if high_degree:
        pb.add_constraint(h3 - a0 * a3 * a2)
    pb.add_constraint(u - t0 * t1)
    if high_degree:
        pb.add_constraint(v - t0 * t1 * a2)
    cols = [(1, main0 + k) for k in range(N_MAIN + pad)]
    return ap.Component(log, pb.build(), cols, log_constraint_degree_bound=bound)


def readers_of(log, offsets, row):
    """The natural rows whose window reads cell `row` of a column sampled at `offsets`: {(row - o) mod N}"""
    n = 1 << log
    return sorted({(row - int(o)) % n for o in offsets})


def drive(logs, offsets="STD", seed=3, lcd=1, bounds=None, high_degree=False, pad=0):
    """Window components of the given sizes + the committed columns, after test_prover_session_cpu.build_mixed_air: mix_u64(len(logs)),
    one dummy preprocessed column claimed by component 0 with mask [0], one main tree, no interaction tree.
    Returns (run(session, commit, tamper=None, alter_mask=False) -> components, tree_logs).
    tamper: (component, natural row) — that cell of the component's `a` is changed.  alter_mask: component 0 is presented with the first
    entry of a's mask moved by one (the verifier's side of a wrong statement)."""
    import nexus_zkvm_amd.air_program as ap
    width = N_MAIN + pad

    def run(sess, commit, tamper=None, alter_mask=False):
        sess.mix_u64(len(logs))
        main, comps = [], []
        for i, l in enumerate(logs):
            base, sec = offsets_of(offsets, l)
            nat, fin = window_trace(l, seed + i, base, sec, pad)
            if tamper is not None and tamper[0] == i:
                nat[COL_A][tamper[1]] = (int(nat[COL_A][tamper[1]]) + 1) % P
                fin[COL_A] = O.finalize_column(nat[COL_A])
            main += fin
            bound = bounds[i] if bounds else 0
            hd = high_degree and ((bound if bound else lcd) >= 2)
            if alter_mask and i == 0:
                base = (base[0] + 1,) + tuple(base[1:])
            comps.append(window_component(ap, l, width * i, base, sec, bound, hd, pad))
        commit([np.zeros(1 << logs[0], np.uint32)])                                # a (dummy) preprocessed column
        commit(main)
        c0 = comps[0]
        comps[0] = ap.Component(c0.log_size, c0.program, c0.cols + [(0, 0)], c0.masks + [[0]], c0.log_constraint_degree_bound)
        return comps
    tree_logs = [[logs[0]], [l for l in logs for _ in range(width)]]
    return run, tree_logs


def wide_variant(log, seed=3):
    """The window component with masks a@(-2, +3) only and T at 0, plus PAD free columns claimed at [0]: the largest size group has
    exactly three sample points (0, -2, +3) and enough columns per point for the coefficient quotients."""
    return drive((log,), "WIDE", seed=seed, pad=PAD)


def sample_points_of(components, log):
    """The distinct offsets modulo N at which columns of size `log` are sampled, and the number of such columns claimed."""
    n = 1 << log
    pts, cols = set(), set()
    for c in components:
        if c.log_size != log:
            continue
        for col, m in zip(c.cols, c.masks):
            cols.add(col)
            pts.update(int(o) % n for o in m)
    return sorted(pts), len(cols)


# ---- composition-kernel programs ---------------------------------------------------------------------------------------------------
def window_program(ap, base, sec, fillers=0, late=None):
    """The high-degree window program alone.  fillers: that many degree-2 constraints over offset-0 reads in front (a long program for the
    segment budget).  late: an offset read only by one further constraint at the very end (the last segment is the first to use it)."""
    pb = ap.ProgramBuilder()
    a0, a1, a2, a3 = pb.next_trace_mask(COL_A, base)
    (w,) = pb.next_trace_mask(COL_W)
    (h3,) = pb.next_trace_mask(COL_H3)
    (h4,) = pb.next_trace_mask(COL_H4)
    t0, t1 = pb.next_secure_mask(COL_T, sec)
    (u,) = pb.next_secure_mask(COL_U)
    (v,) = pb.next_secure_mask(COL_V)
    for k in range(fillers):
        pb.add_constraint((w + k) * (h3 - k) * u + (h4 * (k + 2) - w) * v)
    pb.add_constraint(h4 - a0 * a3 * a2 * a1)
    pb.add_constraint(w - a0 * a3 - a1 - 5 * a2)
    pb.add_constraint(h3 - a0 * a3 * a2)
    pb.add_constraint(u - t0 * t1)
    pb.add_constraint(v - t0 * t1 * a2)
    if late is not None:
        (x,) = pb.next_trace_mask(COL_W, (late,))
        pb.add_constraint(x * h4 - w)
    return pb.build()


SEGMENT_BUDGET = 200
SEGMENT_BASE, SEGMENT_SEC, SEGMENT_LATE, SEGMENT_FILLERS = (-2, -1, 1, 2), (-3, 2), 3, 2


def segmented_program(ap):
    """Under "air.segment" = 200 at least three kernels; offset +3 occurs only in the last constraint, so the last segment is the first
    whose preamble declares it."""
    return window_program(ap, SEGMENT_BASE, SEGMENT_SEC, fillers=SEGMENT_FILLERS, late=SEGMENT_LATE)


def random_program(ap, rng, n_cols, n_ops, offsets):
    """tests/test_gpu_parity.py::_random_program with the masks drawn from `offsets` instead of -1 / 0 / +1: every opcode."""
    pb = ap.ProgramBuilder()
    offsets = [int(o) for o in offsets]
    pick = lambda k: tuple(offsets[(k + j) % len(offsets)] for j in range(1 + k % 3))
    base = [e for k in range(n_cols - 4) for e in pb.next_trace_mask(k, pick(k))]
    sec = pb.next_secure_mask(n_cols - 4, pick(n_cols))
    sec.append(pb.econst(rng.integers(0, P, 4)))
    for _ in range(n_ops):
        r = rng.integers(0, 8)
        if r < 3:
            a, b = base[rng.integers(len(base))], base[rng.integers(len(base))]
            base.append([a + b, a - b, a * b][r])
        elif r == 3:
            base.append(-base[rng.integers(len(base))] + int(rng.integers(0, P)))
        elif r < 6:
            a, b = sec[rng.integers(len(sec))], sec[rng.integers(len(sec))]
            sec.append([a + b, a * b][r - 4])
        elif r == 6:
            sec.append(sec[rng.integers(len(sec))] * base[rng.integers(len(base))] - sec[rng.integers(len(sec))])
        else:
            sec.append(base[rng.integers(len(base))] - sec[rng.integers(len(sec))] + base[rng.integers(len(base))])
        if rng.integers(0, 3) == 0:
            pb.add_constraint(base[-1] if rng.integers(0, 2) else sec[-1])
    pb.add_constraint(base[-1]); pb.add_constraint(sec[-1])
    return pb.build()


ALL_OFFSETS = sorted({o for s in (STD, FAR(4), FAR(8), FAR(32), COINCIDE, HUGE) for part in s for o in part})
KERNEL_SHAPES = [(log, d) for log in (2, 3, 5, 9) for d in (1, 2, 3)]       # (log_size, log_eval - log_size)


# ---- a relation program that reads at offsets (nx_logup_program) ------------------------------------------------------------------
def relation_program_at_offsets(ap, z, alpha, shift, fillers=0):
    """After air_examples.relation_program (the same 7 main columns a, b, c, d, m, p, q): tuple values at a@-2 and a@+3, a multiplicity
    expression reading q@-3.  fillers: further entries, for a program of several segments."""
    pb = ap.ProgramBuilder()
    a_m2, a, a_p3 = pb.next_trace_mask(0, (-2, 0, 3))
    (b,) = pb.next_trace_mask(1)
    (c,) = pb.next_trace_mask(2)
    (d,) = pb.next_trace_mask(3)
    (m,) = pb.next_trace_mask(4)
    (p,) = pb.next_trace_mask(5)
    q, q_m3 = pb.next_trace_mask(6, (0, -3))
    r3 = pb.relation(z, alpha, 3)
    r2 = pb.relation([int(x) ^ 1 for x in z], alpha, 2)
    pb.add_to_relation(r3, 1, [a, b, c])
    pb.add_to_relation(r3, -m, [a_m2 + 5, d, a_p3])
    pb.add_to_relation(r2, q_m3 - 1, [p, a_m2])
    pb.add_to_relation(r2, q, [a_p3])
    for k in range(fillers):
        pb.add_to_relation(r3, q_m3 + k, [a_p3 * (k + 1), b + k, a_m2])
    pb.finalize_logup_in_pairs(7, shift)
    return pb
