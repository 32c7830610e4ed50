"""The RV32M multiply and divide chips of the v1 machine in plain Python integers: every column the five chips' fill_main_trace
bodies write (reference prover/src/chips/instructions/m/: MulChip, MulhuChip, MulhMulhsuChip, DivuRemuChip, DivRemChip), per row, from
ValueB, ValueC and the opcode.  The algorithm is restated from the arithmetic:

  * the 64-bit product of two words through byte products z_k = x_k y_k and the cross sums p_ij = x_i y_j + x_j y_i, assembled
    16 bits at a time with the carries MulCarry0 .. MulCarry3 (P1 = p_01, P3' = p_03, P3'' = p_12, P5 = p_23, each a half-word and a
    carry bit);
  * division verified as dividend = quotient * divisor + remainder with t = quotient * divisor, r = dividend - t, u = divisor - r - 1
    and the borrows of the two subtractions at bit 16;
  * signed operations on absolute values: |x| = ~x + 1 for a negative x, with the carries of that increment at bits 16 and 32 (48, 64).

The quirks that reach the trace are kept: a zero divisor gives quotient bytes FF FF FF FF, remainder = dividend, HelperU = 0;
i32::MIN / -1 sets IsOverflow; under DIV the quotient's carries feed ValueAAbsBorrow, under REM the remainder's; each chip writes
only its own columns, so a column another opcode's chip fills is 0 on this row.  It is never the library.

The file also holds `interp`, tests/trace_programs.py's interpreter extended by the seven opcodes of the W register kind."""
import numpy as np

import trace_programs as TP

P = TP.P
M32 = 0xFFFFFFFF
OPS = ("mul", "mulhu", "mulh", "mulhsu", "divu", "remu", "div", "rem")
# the operand list of the issue: zero and one, 2^31 and above, both sides of the 24-bit float mantissa, MIN and -1, 64-bit products
E = [0, 1, 2, 3, 0xFF, 0x100, 0xFFFF, 0x10000, 0x10001, 0xFFFFFF, 0x1000000, 0x1000001,
     0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFF0000, 0xFFFF0001, 0xFFFFFFFE, 0xFFFFFFFF, 0x55555555, 0xAAAAAAAB]
PAIRS = [(b, c) for b in E for c in E]

# ---------------------------------------------------------------- the columns ----------
SEEDS = [("ValueB", 4), ("ValueC", 4)] + [("Is" + op.capitalize(), 1) for op in OPS]
DERIVED = [("ValueA", 4), ("SgnA", 1), ("SgnB", 1), ("SgnC", 1),
           ("MulP1", 2), ("MulP3Prime", 2), ("MulP3PrimePrime", 2), ("MulP5", 2),
           ("MulC1", 1), ("MulC3Prime", 1), ("MulC3PrimePrime", 1), ("MulC5", 1),
           ("MulCarry0", 1), ("MulCarry1", 1), ("MulCarry2_0", 1), ("MulCarry2_1", 1), ("MulCarry3", 1),
           ("Quotient", 4), ("HelperT", 4), ("Remainder", 4), ("RemainderBorrow", 1), ("HelperU", 4), ("HelperUBorrow", 1),
           ("IsDivideByZero", 1), ("IsAZero", 1), ("IsOverflow", 1),
           ("ValueAAbs", 4), ("ValueAAbsHigh", 4), ("ValueBAbs", 4), ("ValueCAbs", 4),
           ("ValueAAbsBorrow", 2), ("ValueAAbsBorrowHigh", 2), ("ValueBAbsBorrow", 2), ("ValueCAbsBorrow", 2), ("ValueALow", 4)]
COL, SIZE, N_COLS = {}, {}, 0
for _name, _size in SEEDS + DERIVED:
    COL[_name], SIZE[_name] = N_COLS, _size
    N_COLS += _size
N_SEED = sum(s for _, s in SEEDS)
# what the reference attaches to these columns: bytes (range256), MulCarry1 (range8), booleans
BYTE_COLUMNS = ("ValueA", "ValueB", "ValueC", "HelperT", "HelperU", "Quotient", "Remainder", "ValueBAbs", "ValueCAbs", "ValueAAbs",
                "ValueAAbsHigh", "ValueALow", "MulP1", "MulP3Prime", "MulP3PrimePrime", "MulP5")
BOOL_COLUMNS = tuple(n for n, _ in SEEDS[2:]) + tuple(n for n, _ in DERIVED if n not in BYTE_COLUMNS and n != "MulCarry1")


def cols_of(name):
    return list(range(COL[name], COL[name] + SIZE[name]))


def le_bytes(v, n=4):
    return [(v >> (8 * k)) & 255 for k in range(n)]


# ---------------------------------------------------------------- the arithmetic ----------
def mull(x, y):
    """The 64-bit product with every intermediate value the chips commit."""
    a, b = le_bytes(x), le_bytes(y)
    z = [a[k] * b[k] for k in range(4)]
    cross = lambda i, j: (a[i] + a[j]) * (b[i] + b[j]) - z[i] - z[j]
    p1, p2, p3a, p3b, p4, p5 = cross(0, 1), cross(0, 2), cross(0, 3), cross(1, 2), cross(1, 3), cross(2, 3)
    r = {"c1": p1 >> 16, "c3a": p3a >> 16, "c3b": p3b >> 16, "c5": p5 >> 16}
    p1, p3a, p3b, p5 = p1 & 0xFFFF, p3a & 0xFFFF, p3b & 0xFFFF, p5 & 0xFFFF
    s0 = z[0] + ((p1 & 255) << 8)
    s1 = z[1] + (p1 >> 8) + p2 + (s0 >> 16) + (((p3a & 255) + (p3b & 255) + r["c1"]) << 8)
    s2 = z[2] + p4 + (p3a >> 8) + (p3b >> 8) + ((p5 & 255) << 8) + (s1 >> 16) + ((r["c3a"] + r["c3b"]) << 8)
    s3 = z[3] + (p5 >> 8) + (r["c5"] << 8) + (s2 >> 16)
    carry = [s0 >> 16, s1 >> 16, s2 >> 16, s3 >> 16]
    lo, hi = (s0 & 0xFFFF) | ((s1 & 0xFFFF) << 16), (s2 & 0xFFFF) | ((s3 & 0xFFFF) << 16)
    assert (hi << 32) | lo == x * y, (x, y)
    # the bounds the reference asserts
    assert max(r.values()) < 2 and carry[0] < 2 and carry[1] < 5 and carry[2] < 4 and carry[3] < 2, (x, y)
    r.update(p1=p1, p3a=p3a, p3b=p3b, p5=p5, carry=carry, lo=lo, hi=hi)
    return r


def negate_carries(v, bits=32):
    """(~v + 1, the carries of the increment out of every 16-bit chunk)"""
    out, carries, c = 0, [], 1
    for k in range(bits // 16):
        s = (0xFFFF - ((v >> (16 * k)) & 0xFFFF)) + c
        out |= (s & 0xFFFF) << (16 * k)
        c = s >> 16
        carries.append(c)
    return out, carries


def absolute(v, bits=32):
    """(sign, |v|, the two or four carries the chips commit: 0 for a value that is not negative)"""
    if (v >> (bits - 1)) & 1 == 0:
        return 0, v, [0] * (bits // 16)
    a, carries = negate_carries(v, bits)
    return 1, a, carries


def divide_check(quotient, dividend, divisor):
    """t, r, u and the two low borrows of dividend = quotient * divisor + r, u = divisor - r - 1; a zero divisor: r = dividend, u = 0"""
    if divisor == 0:
        return {"r": dividend, "r_borrow": 0, "u": 0, "u_borrow": 0}
    t = mull(quotient, divisor)
    assert t["hi"] == 0
    r = dividend - t["lo"]
    assert 0 <= r < divisor
    u = divisor - r - 1
    return {"r": r, "r_borrow": int((dividend & 0xFFFF) < (t["lo"] & 0xFFFF)), "u": u, "u_borrow": int((divisor & 0xFFFF) < (r & 0xFFFF) + 1)}


def signed(v):
    return v - (1 << 32) if v >> 31 else v


def row(op, b, c):
    """{column name: list of limb values} of what the chip of `op` writes on a row with these operands; every other column is 0."""
    w = {}

    def put(name, v):
        w[name] = list(v) if isinstance(v, (list, tuple)) else le_bytes(v, SIZE[name]) if SIZE[name] > 1 else [int(v)]

    def put_mull(m, names):
        table = {"MulP1": le_bytes(m["p1"], 2), "MulP3Prime": le_bytes(m["p3a"], 2), "MulP3PrimePrime": le_bytes(m["p3b"], 2), "MulP5": le_bytes(m["p5"], 2),
                 "MulC1": [m["c1"]], "MulC3Prime": [m["c3a"]], "MulC3PrimePrime": [m["c3b"]], "MulC5": [m["c5"]],
                 "MulCarry0": [m["carry"][0]], "MulCarry1": [m["carry"][1]], "MulCarry2_0": [m["carry"][2] & 1], "MulCarry2_1": [m["carry"][2] >> 1],
                 "MulCarry3": [m["carry"][3]]}
        for n in names:
            w[n] = table[n]

    LOW = ("MulCarry0", "MulCarry1", "MulP1", "MulP3Prime", "MulP3PrimePrime", "MulC1", "MulC3Prime", "MulC3PrimePrime")
    HIGH = ("MulCarry1", "MulCarry2_0", "MulCarry2_1", "MulCarry3", "MulP3Prime", "MulP3PrimePrime", "MulP5", "MulC3Prime", "MulC3PrimePrime", "MulC5")
    if op == "mul":
        m = mull(b, c)
        put_mull(m, LOW)
        put("ValueA", m["lo"])
    elif op == "mulhu":
        m = mull(b, c)
        put_mull(m, HIGH)
        put("ValueA", m["hi"])
    elif op in ("mulh", "mulhsu"):
        sb, ab, bb = absolute(b)
        put("ValueBAbs", ab); put("ValueBAbsBorrow", bb); put("SgnB", sb)
        if op == "mulh":
            sc, ac, bc = absolute(c)
            put("ValueCAbsBorrow", bc); put("SgnC", sc)
        else:
            ac = c
        put("ValueCAbs", ac)
        m = mull(ab, ac)
        put_mull(m, set(LOW) | set(HIGH))
        put("ValueAAbs", m["lo"]); put("ValueAAbsHigh", m["hi"])
        put("IsAZero", int(m["lo"] == 0 and m["hi"] == 0))
        product = (signed(b) * (signed(c) if op == "mulh" else c)) & ((1 << 64) - 1)
        sa, _, ba = absolute(product, 64)
        put("SgnA", sa); put("ValueAAbsBorrow", ba[:2]); put("ValueAAbsBorrowHigh", ba[2:])
        put("ValueALow", product & M32); put("ValueA", product >> 32)
    elif op in ("divu", "remu"):
        q, r = (M32, b) if c == 0 else (b // c, b % c)
        put("Quotient", q)
        m = mull(q, c)
        put_mull(m, LOW)
        put("IsDivideByZero", int(c == 0)); put("HelperT", m["lo"])
        d = divide_check(q, b, c)
        assert d["r"] == r
        put("Remainder", d["r"]); put("RemainderBorrow", d["r_borrow"]); put("HelperU", d["u"]); put("HelperUBorrow", d["u_borrow"])
        put("ValueA", q if op == "divu" else r)
    else:
        sb, ab, bb = absolute(b)
        sc, ac, bc = absolute(c)
        if c == 0:
            value_q, value_r = M32, b
            aq, rem_abs, carries_q, carries_r = M32, ab, [0, 0], bb
        elif b == 0x80000000 and c == M32:
            value_q, value_r = 0x80000000, 0
            aq, rem_abs, carries_q, carries_r = 0x80000000, 0, [0, 0], [0, 0]
        else:
            qs = abs(signed(b)) // abs(signed(c)) * (-1 if sb != sc else 1)           # RISC-V: the quotient rounds towards zero
            rs = signed(b) - qs * signed(c)
            value_q, value_r = qs & M32, rs & M32
            _, aq, carries_q = absolute(value_q)
            _, rem_abs, carries_r = absolute(value_r)
        put("IsDivideByZero", int(c == 0)); put("IsOverflow", int(b == 0x80000000 and c == M32))
        put("Quotient", aq)
        put("ValueAAbsBorrow", carries_q if op == "div" else carries_r)
        put("ValueBAbs", ab); put("ValueBAbsBorrow", bb); put("ValueCAbs", ac); put("ValueCAbsBorrow", bc)
        m = mull(aq, ac)
        put_mull(m, LOW)
        put("HelperT", m["lo"])
        d = divide_check(aq, ab, ac)
        assert d["r"] == rem_abs
        put("Remainder", d["r"]); put("RemainderBorrow", d["r_borrow"]); put("HelperU", d["u"]); put("HelperUBorrow", d["u_borrow"])
        value_a = value_q if op == "div" else value_r
        put("ValueA", value_a); put("SgnA", value_a >> 31); put("SgnB", sb); put("SgnC", sc); put("IsAZero", int(value_a == 0))
    return w


# ---------------------------------------------------------------- a trace ----------
LOG = 9
SENTINEL = 0x12345678


def trace_ops(op, log_size=LOG):
    """The opcode of every natural row: the 441 pairs as rows of `op`, the rest rows of other opcodes (None).  Smaller traces take the
    pairs at a stride, so that a zero divisor and the large operands stay in."""
    n = 1 << log_size
    if n > len(PAIRS):
        return [op] * len(PAIRS) + [None] * (n - len(PAIRS)), PAIRS + [(7 * k + 1, 5 * k) for k in range(n - len(PAIRS))]
    step = len(PAIRS) // n
    return [op] * (n - 1) + [None], [PAIRS[k * step] for k in range(n)]


def seeds_and_trace(ops, operands, sentinel=SENTINEL):
    """(the N_COLS natural-order uint64 columns before the fill: seeds, the sentinel in ValueA, 0 elsewhere; the columns the model
    expects after it)"""
    n = len(ops)
    before = [np.zeros(n, np.uint64) for _ in range(N_COLS)]
    for k in cols_of("ValueA"):
        before[k][:] = sentinel
    for i, (op, (b, c)) in enumerate(zip(ops, operands)):
        for k in range(4):
            before[COL["ValueB"] + k][i], before[COL["ValueC"] + k][i] = (b >> (8 * k)) & 255, (c >> (8 * k)) & 255
        if op is not None:
            before[COL["Is" + op.capitalize()]][i] = 1
    after = [x.copy() for x in before]
    for i, (op, (b, c)) in enumerate(zip(ops, operands)):
        if op is None:
            continue
        for name, limbs in row(op, b, c).items():
            assert len(limbs) == SIZE[name], name
            for k, v in enumerate(limbs):
                after[COL[name] + k][i] = v
    return before, after


# ---------------------------------------------------------------- the interpreter of the W opcodes ----------
def interp(program, cols_nat, log_size):
    """tests/trace_programs.py's `interp` with the W register kind: the field opcodes run there, one instruction at a time, the seven
    integer opcodes here on Python integers.  Natural-order columns in, natural-order columns out."""
    import nexus_zkvm_amd.air_program as ap
    n = 1 << log_size
    rows = np.arange(n)
    cols = [None if c is None else np.array(c, np.uint64) for c in cols_nat]
    before = [None if c is None else c.copy() for c in cols]
    R = [None] * program.n_regs
    obj = lambda f, x, y: np.array([f(int(u), int(v)) for u, v in zip(x, y)], np.uint64)
    W = {ap.T_PACK32: lambda u, v: (u + (v << 16)) & M32, ap.T_MULLO32: lambda u, v: (u * v) & M32, ap.T_MULHU32: lambda u, v: (u * v) >> 32,
         ap.T_DIVU32: lambda u, v: u // v if v else M32, ap.T_REMU32: lambda u, v: u % v if v else u}
    base = ap.Program(None, program.n_regs, None, 0)
    for op, dst, a, b in np.asarray(program.instrs, np.uint32).reshape(-1, 4).tolist():
        if op in W:
            R[dst] = obj(W[op], R[a], R[b])
        elif op == ap.T_LO16:
            R[dst] = R[a] & np.uint64(0xFFFF)
        elif op == ap.T_HI16:
            R[dst] = R[a] >> np.uint64(16)
        elif op == ap.LOAD:
            R[dst] = before[a][(rows + int(np.int32(np.uint32(b)))) % n]
        elif op == ap.T_STORE:
            cols[a] = R[b].copy()
        elif op == ap.T_STORE_IF:
            cols[a] = np.where(R[dst] != 0, R[b], cols[a])
        else:
            # one field instruction through the interpreter it belongs to: its operands as two input columns, its result stored
            srcs = [] if op in (ap.CONST, ap.T_ROW) else [a] if op in (ap.NEG, ap.T_INV) else [a, b]
            ins = [R[s] if R[s] is not None else np.zeros(n, np.uint64) for s in srcs]
            prog = [(ap.LOAD, k, k, 0) for k in range(len(ins))] + [(op, 2, a if not srcs else 0, b if not srcs else 1), (ap.T_STORE, 0, 2, 2)]
            base.instrs, base.n_regs = np.array(prog, np.uint32), 3
            R[dst] = TP.interp(base, ins + [np.zeros(n, np.uint64)] * (3 - len(ins)), log_size)[2]
    return cols
