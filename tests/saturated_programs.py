"""Hand-written AIR programs and operand sets for the lazily reduced field sums (shared by tests/test_gpu_saturated.py and
tests/test_air_text_host_cpu.py).

The rule under test (csrc/field.cuh): products of canonical M31 words are added as raw 64-bit integers and folded after at most FOUR
of them, 4 (p-1)^2 + 2^33 + 2^31 < 2^64; five do not fit.  Uniformly random words never come near that bound, so the programs here are
run on
    SAT   every word p-1, and
    EDGE  words from {0, 1, p-1, p-2}, "enumerated" = every combination laid out over the rows.
The programs are instruction arrays, not recorded ones: the recorder never emits the in-place `ADDE D,D,T` the dot-product peephole of
csrc/air_jit.hip looks for.  The reference is interp() below: numpy uint64, every sum and product reduced at once."""
import numpy as np

import nexus_zkvm_amd.air_program as ap

P = ap.P
EDGE = np.array([0, 1, P - 1, P - 2], np.uint32)
N_COLS, N_ECONSTS = 8, 3            # what the chains, guards and runs programs load: column k % 8, secure constant k % 3
CHAIN_TERMS = (1, 3, 4, 5, 8, 9, 200)


class Asm:
    """A straight-line program written by hand.  Registers are handed out in order and never reused unless the caller says so; a secure
    value is 4 consecutive registers.  mode "cons": the roots are constraints; "frac": the same values are the denominators (or base-field
    numerators) of logup fractions, one logup column each, which is what nx_logup_program takes."""

    def __init__(self, mode="cons"):
        self.mode, self.ins, self.n_regs, self.n_roots = mode, [], 0, 0
        self.marks = {}                             # name -> register of a value a test wants to find in the generated text
        self.num_b = self.num_e = self.den_e = None

    def b(self):
        self.n_regs += 1
        return self.n_regs - 1

    def e(self):
        self.n_regs += 4
        return self.n_regs - 4

    def op(self, op, dst, a=0, b=0):
        self.ins.append((op, dst, a, b))

    def prologue(self):
        """frac mode: a base-field numerator (p-1 under SAT), a secure numerator and a secure denominator for base-field roots"""
        if self.mode != "frac":
            return
        self.num_b, self.num_e, self.den_e, c = self.b(), self.e(), self.e(), self.b()
        self.op(ap.LOAD, self.num_b, 0, 0)
        self.op(ap.CONSTE, self.num_e, 1)
        self.op(ap.CONSTE, self.den_e, 2)
        self.op(ap.CONST, c, 11)
        self.op(ap.ADDEB, self.den_e, self.den_e, c)

    def root_e(self, reg):
        if self.mode == "cons":
            self.op(ap.CONSTRAINT_E, 0, reg, 0)
        elif self.n_roots % 2:
            self.op(ap.FRAC, self.n_roots, self.num_e, reg)
        else:
            self.op(ap.FRACB, self.n_roots, self.num_b, reg)
        self.n_roots += 1

    def root_b(self, reg):
        if self.mode == "cons":
            self.op(ap.CONSTRAINT_B, 0, reg, 0)
        else:
            self.op(ap.FRACB, self.n_roots, reg, self.den_e)
        self.n_roots += 1

    def program(self, econsts):
        ins = np.array(self.ins, dtype=np.uint32).reshape(-1, 4)
        pr = ap.Program(ins, self.n_regs, np.asarray(econsts, np.uint32).reshape(-1, 4), self.n_roots if self.mode == "cons" else 0)
        if self.mode == "frac":
            pr.n_logup_cols = self.n_roots
        return pr


class _Chains:
    """sum_k A_k v_k into D, one `CONSTE A; LOAD v; MULEB T,A,v; ADDE D,D,T` per term (order 1: `ADDE D,T,D`).  A, v and T are shared
    by every chain: each is rewritten before it is read again, so T is dead after its ADDE — the shape the peephole fuses."""

    def __init__(self, a):
        self.a, self.A, self.T, self.v, self.k = a, a.e(), a.e(), a.b(), 0
        self.c7 = a.b()
        a.op(ap.CONST, self.c7, 7)

    def start(self, D=None):
        """D = (p-1 + 7, p-1, p-1, p-1) under SAT: k terms later it is (k + 6, k - 1, k - 1, k - 1) — never zero for k <= 200, so
        every root is a failing constraint for air_check and an invertible denominator for the fraction form"""
        a = self.a
        D = a.e() if D is None else D
        a.op(ap.CONSTE, D, 0)
        a.op(ap.ADDEB, D, D, self.c7)
        return D

    def term(self, D, order=0, A=None, v=None, T=None, load=True, const=True):
        a = self.a
        A, v, T = self.A if A is None else A, self.v if v is None else v, self.T if T is None else T
        if const:
            a.op(ap.CONSTE, A, self.k % N_ECONSTS)
        if load:
            a.op(ap.LOAD, v, self.k % N_COLS, 0)
        a.op(ap.MULEB, T, A, v)
        if order == 0:
            a.op(ap.ADDE, D, D, T)
        else:
            a.op(ap.ADDE, D, T, D)
        self.k += 1


def chains_program(mode="cons", pinned=False):
    """Program A: in-place dot chains of 1, 3, 4, 5, 8, 9 and 200 terms in both operand orders of the ADDE, one root each.
    pinned: every root D is followed by the root D - K_j, K_j = secure constant N_ECONSTS + j — zero exactly when the chain's sum is
    the constant's value (the form a trace checker can see a wrong sum in: it reports which constraints are not zero, and where)."""
    a = Asm(mode)
    a.prologue()
    _emit_chains(a, _Chains(a), pinned)
    return a


def _emit_chains(a, ch, pinned=False):
    K = a.e() if pinned else None
    j = 0
    for order in (0, 1):
        for n in CHAIN_TERMS:
            D = ch.start()
            for _ in range(n):
                ch.term(D, order)
            a.root_e(D)
            if pinned:
                a.op(ap.CONSTE, K, N_ECONSTS + j)
                a.op(ap.SUBE, K, D, K)
                a.root_e(K)
            j += 1


def pinned_chain_econsts():
    """SAT constants followed by the value of every chain of program A under SAT operands (from interp)"""
    plain = chains_program().program(sat_econsts())
    cons, _ = interp(plain, np.full((N_COLS, 1), P - 1, np.uint32))
    return np.concatenate([sat_econsts(), np.array([[int(c[k][0]) for k in range(4)] for c in cons], np.uint32)])


def guards_program(mode="cons", runs=False):
    """Program B: what the peephole's guards are for; with runs=True followed by program C's constraint runs.
    Compiled with a small "air.segment" that longer program is several kernels: a cut falls between the two roots of the
    materialise-and-restart chain (the second kernel sums the whole chain again) and inside the run of consecutive CONSTRAINT_B."""
    a = Asm(mode)
    a.prologue()
    es = _emit_guards(a, _Chains(a))
    if mode == "cons" and runs:
        _runs(a, es)
    return a


def all_program(mode="cons", pinned=False, runs=False):
    """Programs A and B (and C) in one: one compilation where the generated kernel is what costs the time.  The chains come first, so
    pinned_chain_econsts() fits this program too."""
    a = Asm(mode)
    a.prologue()
    ch = _Chains(a)
    _emit_chains(a, ch, pinned)
    es = _emit_guards(a, ch)
    if mode == "cons" and runs:
        _runs(a, es)
    return a


def _emit_guards(a, ch):
    # 1. two chains interleaved: two accumulators pending together, 9 terms each
    D1, D2 = ch.start(), ch.start()
    for _ in range(9):
        ch.term(D1, 0)
        ch.term(D2, 1)
    a.root_e(D1); a.root_e(D2)
    # 2. D read by a MULE after 5 terms (materialise), then continued (restart) for 5 more
    D3, M = ch.start(), a.e()
    for _ in range(5):
        ch.term(D3)
    a.op(ap.MULE, M, D3, D3)
    for _ in range(5):
        ch.term(D3)
    a.root_e(M); a.root_e(D3)
    a.marks["D3"] = D3
    # 3. the factors of a term are another chain's pending accumulator: A = D4 (all four words), then v = one word of D4
    D4, D5 = ch.start(), ch.start()
    for _ in range(5):
        ch.term(D4)
    ch.term(D5, A=D4, const=False)
    for _ in range(5):
        ch.term(D4)
    ch.term(D5, v=D4 + 1, load=False)
    for _ in range(3):
        ch.term(D5)
    a.root_e(D4); a.root_e(D5)
    # 4. shapes that must NOT be fused (6 terms each: fused by mistake they would still be summed lazily)
    D6 = a.e()                                    # T is D itself: ADDE D,D,D
    for _ in range(6):
        ch.term(D6, T=D6)
    a.root_e(D6)
    X = a.e(); a.e()                              # T overlaps the upper half of D
    ch.start(X)
    for _ in range(6):
        ch.term(X, T=X + 2)
    a.root_e(X)
    D8 = ch.start()                               # T is A
    for _ in range(6):
        ch.term(D8, T=ch.A)
    a.root_e(D8)
    D8b, A2 = ch.start(), a.e(); a.e()            # T overlaps the upper half of A
    for _ in range(6):
        ch.term(D8b, A=A2, T=A2 + 2)
    a.root_e(D8b)
    D9, S, T9 = ch.start(), ch.start(), a.e()     # T read again later: by another sum (3 terms), not at all (5 terms: fused), by a root (the last)
    for _ in range(3):
        ch.term(D9, T=T9)
        a.op(ap.ADDE, S, S, T9)
    for _ in range(6):
        ch.term(D9, T=T9)
    a.root_e(T9); a.root_e(D9); a.root_e(S)
    D10 = ch.start()                              # v is a word of D
    for _ in range(6):
        ch.term(D10, v=D10 + 2, load=False)
    a.root_e(D10)
    D11, T11 = ch.start(), a.e()                  # v is a word of T
    for _ in range(6):
        ch.term(D11, v=T11 + 1, T=T11)
    a.root_e(D11)
    D12 = ch.start()                              # A is D (times the constant 7: times a saturated word D + D (p-1) would be 0)
    for _ in range(6):
        ch.term(D12, A=D12, const=False, v=ch.c7, load=False)
    a.root_e(D12)
    return [D1, D2, M, D3]


def _runs(a, es):
    """The constraint accumulator's own fold schedule: nine consecutive CONSTRAINT_B on saturated words (a column word times 1: the
    multiplication only makes the slice of each constraint dear enough for a small segment budget to cut the run in two), then
    CONSTRAINT_B and CONSTRAINT_E alternating for 9 (a secure constraint adds a canonical word and counts like a product)."""
    one, bs = a.b(), [a.b() for _ in range(9)]
    a.op(ap.CONST, one, 1)
    for k, r in enumerate(bs):
        a.op(ap.LOAD, r, k % N_COLS, 0)
        a.op(ap.MUL, r, r, one)
    for r in bs:
        a.root_b(r)
    for k in range(9):
        if k % 2 == 0:
            a.root_b(bs[k])
        else:
            a.root_e(es[k // 2])


def runs_program():
    """Program C: the runs alone — no chain, so only the constraint sum's folds are at stake"""
    a = Asm("cons")
    ch = _Chains(a)
    _runs(a, [ch.start() for _ in range(4)])
    return a


def sat_inputs(program, n_rows, n_cols=N_COLS):
    """SAT columns, secure constants and alpha powers of a hand-written program"""
    cols = np.full((n_cols, n_rows), P - 1, np.uint32)
    pw = np.full((max(1, program.n_constraints), 4), P - 1, np.uint32)
    return cols, pw


def sat_econsts(n=N_ECONSTS):
    return np.full((n, 4), P - 1, np.uint32)


# ---- enumerated EDGE operands ------------------------------------------------------------------------------------------------------
def edge_enum(n_coords, n_rows=None):
    """n_coords columns over 4^n_coords rows (or n_rows, the pattern repeating): every combination of EDGE words"""
    n = 4 ** n_coords if n_rows is None else n_rows
    r = np.arange(n, dtype=np.uint64)
    return np.stack([EDGE[((r >> np.uint64(2 * c)) & np.uint64(3)).astype(np.int64)] for c in range(n_coords)]).astype(np.uint32)


def mul_program():
    """x = LOADE 0..3; y = LOADE 4..7; MULE; CONSTRAINT_E: q_mul of field.cuh in the interpreter, the prelude's copy in the JIT (and
    once more each for the alpha power of the constraint)"""
    a = Asm("cons")
    x, y, m = a.e(), a.e(), a.e()
    a.op(ap.LOADE, x, 0, 0)
    a.op(ap.LOADE, y, 4, 0)
    a.op(ap.MULE, m, x, y)
    a.root_e(m)
    return a.program(np.zeros((0, 4), np.uint32))


def frac_program():
    """den = LOADE 0..3; FRAC num = LOADE 4..7 (column 0), FRACB num = LOAD 8 (column 1): q_norm, q_inv_from, q_frac_add and q_mul of
    the logup prelude, with the all-zero denominator among the rows"""
    a = Asm("frac")
    d, n, b = a.e(), a.e(), a.b()
    a.op(ap.LOADE, d, 0, 0)
    a.op(ap.LOADE, n, 4, 0)
    a.op(ap.FRAC, 0, n, d)
    a.op(ap.LOAD, b, 8, 0)
    a.op(ap.FRACB, 1, b, d)
    a.n_roots = 2
    return a.program(np.zeros((0, 4), np.uint32))


def frac_columns(n_coords=8):
    """the 9 columns of frac_program: 8 enumerated coordinates (denominator, numerator) and a base-field numerator from EDGE"""
    cols = edge_enum(n_coords)
    if n_coords < 8:                # a shorter enumeration: the numerator's upper coordinates repeat its lower ones
        cols = np.concatenate([cols, cols[4:4 + (8 - n_coords)]])
    r = np.arange(cols.shape[1])
    return np.concatenate([cols, EDGE[((r >> 8) ^ (r >> 3) ^ r) & 3][None, :]]).astype(np.uint32)


# ---- the reference: every operation reduced at once ---------------------------------------------------------------------------------
def qmul(x, y):
    """(x0 + x1 i + (x2 + x3 i) u)(y0 + ...), i^2 = -1, u^2 = 2 + i, on lists of uint64 arrays (or Python integers)"""
    def cmul(p, q):
        return ((p[0] * q[0] % P + P - p[1] * q[1] % P) % P, (p[0] * q[1] % P + p[1] * q[0] % P) % P)
    a, b, c, d = (x[0], x[1]), (x[2], x[3]), (y[0], y[1]), (y[2], y[3])
    ac, bd, ad, bc = cmul(a, c), cmul(b, d), cmul(a, d), cmul(b, c)
    r = ((2 * bd[0] + P - bd[1]) % P, (2 * bd[1] + bd[0]) % P)
    return [(ac[0] + r[0]) % P, (ac[1] + r[1]) % P, (ad[0] + bc[0]) % P, (ad[1] + bc[1]) % P]


def interp(program, cols, econsts=None):
    """The program on every row of `cols` (offset-0 loads only, so rows are independent).  Returns (constraints, fractions):
    constraints = [4 coordinate arrays per constraint], fractions = [(logup column, numerator 4 arrays, denominator 4 arrays)]."""
    n = cols.shape[1]
    ec = np.asarray(program.econsts if econsts is None else econsts, np.uint64).reshape(-1, 4)
    c64 = cols.astype(np.uint64)
    Z = np.zeros(n, np.uint64)
    R = [Z] * (program.n_regs + 4)
    E = lambda i: list(R[i:i + 4])
    cons, fracs = [], []
    for op, dst, a, b in np.asarray(program.instrs, np.uint32).reshape(-1, 4).tolist():
        if op in (ap.LOAD, ap.LOADE):
            assert b == 0, "the hand-written programs read the current row only"
        if op == ap.LOAD:
            R[dst] = c64[a]
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
        elif op == ap.CONSTE:
            R[dst:dst + 4] = [np.full(n, int(ec[a][k]), np.uint64) for k in range(4)]
        elif op == ap.ADDE:
            R[dst:dst + 4] = [(x + y) % P for x, y in zip(E(a), E(b))]
        elif op == ap.SUBE:
            R[dst:dst + 4] = [(x + P - y) % P for x, y in zip(E(a), E(b))]
        elif op == ap.MULE:
            R[dst:dst + 4] = qmul(E(a), E(b))
        elif op == ap.MULEB:
            s = R[b]
            R[dst:dst + 4] = [(x * s) % P for x in E(a)]
        elif op == ap.ADDEB:
            v = E(a)
            R[dst:dst + 4] = [(v[0] + R[b]) % P, v[1], v[2], v[3]]
        elif op == ap.LOADE:
            R[dst:dst + 4] = [c64[a + k] for k in range(4)]
        elif op == ap.CONSTRAINT_B:
            cons.append([R[a], Z, Z, Z])
        elif op == ap.CONSTRAINT_E:
            cons.append(E(a))
        elif op == ap.FRAC:
            fracs.append((dst, E(a), E(b)))
        elif op == ap.FRACB:
            fracs.append((dst, [R[a], Z, Z, Z], E(b)))
        else:
            raise AssertionError(f"opcode {op}")
    return cons, fracs


def accumulate(cons, pw, denom_inv, log_size, start):
    """start + denom_inv[row >> log_size] * sum_j pw_j C_j(row): what nx_eval_constraint_program / nx_air_eval leave in the accumulator"""
    n = len(start[0])
    pw = np.asarray(pw, np.uint64).reshape(-1, 4)
    s = [np.zeros(n, np.uint64) for _ in range(4)]
    for j, c in enumerate(cons):
        t = qmul([np.full(n, int(pw[j][k]), np.uint64) for k in range(4)], c)
        s = [(x + y) % P for x, y in zip(s, t)]
    di = np.asarray(denom_inv, np.uint64)[np.arange(n) >> log_size]
    return np.stack([(np.asarray(start[k], np.uint64) + s[k] * di % P) % P for k in range(4)]).astype(np.uint32)
