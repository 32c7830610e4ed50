"""Trace programs (nx_trace_program) for the CPU and GPU suites, and the judge of both: `interp`, a numpy interpreter over
NATURAL-order columns that reduces every operation at once.  A LOAD at offset o of row i reads row (i + o) mod N; stores apply in
program order; a column the program does not store keeps every word.  The mapping to the stored order (bit-reversed circle-domain
order) is the permutation of tests/test_trace_check_cpu.py.  It is never the library."""
import numpy as np

from test_trace_check_cpu import natural_row_of_pos

P = (1 << 31) - 1
# every operand the opcode table runs on: shift counts 0, 31, 32 and p-1; OR / XOR / SHL results that reach p
EDGE = [0, 1, 2, 31, 32, 255, 256, 1 << 16, 1 << 30, P - 2, P - 1]
BINARY = ("band", "bor", "bxor", "shl", "shr", "ltu", "eq")


def _ap():
    import nexus_zkvm_amd.air_program as ap
    return ap


def to_storage(nat):
    """A natural-order column in the stored order."""
    nat = np.asarray(nat)
    return nat[natural_row_of_pos(int(np.log2(len(nat))))]


def _inv(a):
    """a^(p-2) mod p, vectorised: the M31 inverse, 0 for 0"""
    r, b, e = np.ones_like(a), a.copy(), P - 2
    while e:
        if e & 1:
            r = (r * b) % P
        b = (b * b) % P
        e >>= 1
    return np.where(a == 0, 0, r).astype(np.uint64)


def interp(program, cols_nat, log_size):
    """The columns after the program ran on every row: a list like cols_nat (natural order, uint64; None stays None)."""
    ap = _ap()
    n = 1 << log_size
    rows = np.arange(n)
    cols = [None if c is None else np.array(c, np.uint64) for c in cols_nat]
    before = [None if c is None else c.copy() for c in cols]
    R = [None] * program.n_regs
    M32 = np.uint64(0xFFFFFFFF)
    for op, dst, a, b in np.asarray(program.instrs, np.uint32).reshape(-1, 4).tolist():
        if op == ap.LOAD:
            R[dst] = before[a][(rows + int(np.int32(np.uint32(b)))) % n]          # a loaded column is never a stored one
        elif op == ap.CONST:
            R[dst] = np.full(n, a, np.uint64)
        elif op == ap.ADD:
            R[dst] = (R[a] + R[b]) % P
        elif op == ap.SUB:
            R[dst] = (R[a] + P - R[b]) % P
        elif op == ap.MUL:
            R[dst] = (R[a] * R[b]) % P
        elif op == ap.NEG:
            R[dst] = (P - R[a]) % P
        elif op == ap.T_ROW:
            R[dst] = rows.astype(np.uint64)
        elif op == ap.T_AND:
            R[dst] = R[a] & R[b]
        elif op == ap.T_OR:
            R[dst] = (R[a] | R[b]) % P
        elif op == ap.T_XOR:
            R[dst] = (R[a] ^ R[b]) % P
        elif op == ap.T_SHL:
            R[dst] = np.where(R[b] < 32, (R[a] << np.minimum(R[b], 31)) & M32, 0).astype(np.uint64) % P
        elif op == ap.T_SHR:
            R[dst] = np.where(R[b] < 32, R[a] >> np.minimum(R[b], 31), 0).astype(np.uint64)
        elif op == ap.T_LTU:
            R[dst] = (R[a] < R[b]).astype(np.uint64)
        elif op == ap.T_EQ:
            R[dst] = (R[a] == R[b]).astype(np.uint64)
        elif op == ap.T_INV:
            R[dst] = _inv(R[a])
        elif op == ap.T_STORE:
            cols[a] = R[b].copy()
        elif op == ap.T_STORE_IF:
            cols[a] = np.where(R[dst] != 0, R[b], cols[a])
        else:
            raise AssertionError(f"opcode {op}")
        assert R[dst] is None or (op in (ap.T_STORE, ap.T_STORE_IF)) or int(R[dst].max()) < P
    return cols


# ---------------------------------------------------------------- the programs ----------
def opcode_table():
    """Every new opcode on all ordered pairs of EDGE: column 0 walks through EDGE along the rows (>= 11 rows), the second operand is
    each of the 11 values as a constant; then the same opcodes on two columns, and INV (of 0, 1 and p-1 among the others).
    Returns (program, n_cols, n_inputs): columns 0, 1 are inputs, the rest one stored column each — 85 stores."""
    pb = _ap().ProgramBuilder()
    (x,), (y,) = pb.next_trace_mask(0), pb.next_trace_mask(1)
    col = 2
    for name in BINARY:
        f = getattr(pb, name)
        for c in EDGE:
            pb.store(col, f(x, pb.const(c)))
            col += 1
        pb.store(col, f(x, y))
        col += 1
    pb.store(col, pb.inv(x))
    return pb.build_trace_program(), col + 1, 2


def opcode_table_inputs(log_size):
    i = np.arange(1 << log_size)
    e = np.array(EDGE, np.uint64)
    return [e[i % 11], e[(i // 11 + 3 * i) % 11]]


OFFSETS = (-2, -1, 1, 3)


def offsets_program():
    """Column 0 at offsets -2, -1, +1, +3 and ROW: columns 1..4 the four neighbours, 5 the row, 6 a value that needs all of them."""
    pb = _ap().ProgramBuilder()
    m2, m1, p1, p3 = pb.next_trace_mask(0, OFFSETS)
    for k, v in enumerate((m2, m1, p1, p3)):
        pb.store(1 + k, v)
    pb.store(5, pb.row())
    pb.store(6, m2 * p3 + pb.bxor(m1, p1) + pb.row())
    return pb.build_trace_program(), 7, 1


def store_if_program():
    """Three "chips" write column 5 under the disjoint flags of columns 1..3, the flag of column 4 (all 0) writes nothing."""
    pb = _ap().ProgramBuilder()
    (x,) = pb.next_trace_mask(0)
    f = [pb.next_trace_mask(1 + k)[0] for k in range(4)]
    pb.store_if(f[0], 5, x + 1)
    pb.store_if(f[1], 5, pb.shl(x, 1))
    pb.store_if(f[2], 5, pb.bxor(x, 5))
    pb.store_if(f[3], 5, pb.const(77))
    return pb.build_trace_program(), 6, 5


SENTINEL = 0x12345678


def store_if_inputs(log_size, seed=3):
    """x, the four flags (row i belongs to chip i % 4; chip 3 has no flag set: its rows keep the sentinel), the shared column"""
    n = 1 << log_size
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 16, n).astype(np.uint64)
    owner = np.arange(n) % 4
    return [x] + [(owner == k).astype(np.uint64) for k in range(3)] + [np.zeros(n, np.uint64), np.full(n, SENTINEL, np.uint64)]
