"""A recorded AIR with one constraint of every degree 1 .. 5 in every form the composition planner tells apart, with valid traces: the
statement of tests/test_degree_ladder_cpu.py and tests/test_gpu_degree_ladder.py.  Plain data and small helpers, in the manner of
tests/wide_mask_air.py.

The planner of csrc/prover.hip (prepare_component_kernels) places a constraint by its ESTIMATED degree (nx_air_constraint_degrees: loads 1,
constants 0, sums the larger, products the sum): <= 2 on the first half of the committed domain, 3 on the 2N-point domain, 4 on the
committed 2N rows plus a quarter of the 4N-point domain, the rest on the component's own domain.  Each placement is exact only up to a
degree, so every form below is written once per degree it can reach; the constraint is always `result - expression`, the result column
filled with the expression's value, so the constraint vanishes on the trace and its quotient has degree (d - 1) N exactly.

    base columns (12):  x0 .. x5 | one (all ones) | s (a 0 / 1 selector) | T (4 coordinates)
    then one result column per base constraint, four per secure one, in constraint order

    plain  d = 1 .. 6   x0 x1 ... x(d-1)                                       d loads at offset 0 (NX_C_MUL); 6 only in "d6"
    sel    d = 2 .. 5   s (x0 ... x(d-2) + x5 + 3)                             a flag times a sum: the RV32M chips' shape
    next   d = 1 .. 5   x0@+1 x1 ... x(d-1)                                    one factor at the next row
    prev   d = 1 .. 5   x0 ... x(d-2) x(d-1)@-1                                one factor at the previous row
    secb   d = 2 .. 5   T x0 ... x(d-2)                                        secure times base (NX_C_MULEB)
    sece   d = 2 .. 5   T T | T T T | (T T)(T T) | (T T)(T T) T                secure times secure (NX_C_MULE)
    top    d = 1 .. 5   x0 ... x(d-1) + sum_k (k + 1) x5 x4 ... x(6-k) + 11    the max rule: lower-degree terms and a constant beside the top
    over   estimated 5  x0 x1 x2 x3 one                                        true degree 4: `one` is a constant polynomial

x@o is row (i + o) mod N of the natural trace order."""
from functools import reduce

import numpy as np

import oracle_lib as O
from wide_mask_air import at, qmul_rows

P = O.P
N_X = 6
COL_ONE, COL_S, COL_T, N_BASE = 6, 7, 8, 12
SECURE_FORMS = ("secb", "sece")


def _prod(fs):
    return reduce(lambda a, b: a * b, fs)


def _sece(c, d):
    t = c.T()
    return {2: lambda: t * t, 3: lambda: t * t * t, 4: lambda: (t * t) * (t * t), 5: lambda: (t * t) * (t * t) * t}[d]()


# form -> (the degrees it is written at, expression(c, d)); c hands out the columns (numbers for the trace, recorded values for the program)
FORMS = {
    "plain": ((1, 2, 3, 4, 5, 6), lambda c, d: _prod([c.x(i) for i in range(d)])),
    "sel": ((2, 3, 4, 5), lambda c, d: c.s() * (_prod([c.x(i) for i in range(d - 1)]) + c.x(5) + 3)),
    "next": ((1, 2, 3, 4, 5), lambda c, d: _prod([c.x(0, 1)] + [c.x(i) for i in range(1, d)])),
    "prev": ((1, 2, 3, 4, 5), lambda c, d: _prod([c.x(i) for i in range(d - 1)] + [c.x(d - 1, -1)])),
    "secb": ((2, 3, 4, 5), lambda c, d: _prod([c.T()] + [c.x(i) for i in range(d - 1)])),
    "sece": ((2, 3, 4, 5), _sece),
    "top": ((1, 2, 3, 4, 5), lambda c, d: reduce(lambda a, b: a + b, [_prod([c.x(i) for i in range(d)])]
                                                   + [(k + 1) * _prod([c.x(5 - i) for i in range(k)]) for k in range(1, d)]) + 11),
    "over": ((5,), lambda c, d: c.x(0) * c.x(1) * c.x(2) * c.x(3) * c.one()),
}
# (name, form, the degree nx_air_constraint_degrees gives, the true degree), form-major: in "mixed" the degrees interleave
CONSTRAINTS = [(f"{form}{d}", form, d, 4 if form == "over" else d) for form, (degrees, _) in FORMS.items() for d in degrees]
MAX_PROVABLE = 5                               # log_constraint_degree_bound 2: the quotient of a degree-5 constraint fills the 4N-point space


def constraints_of(kind):
    """The constraints of a component kind: "d1" .. "d6" only those of that (estimated) degree; "mixed" all up to degree 5; "low" those of
    "mixed" up to degree 3 (what a bound of 1 admits)."""
    if kind == "mixed":
        return [c for c in CONSTRAINTS if c[2] <= MAX_PROVABLE]
    if kind == "low":
        return [c for c in CONSTRAINTS if c[2] <= 3]
    assert kind[0] == "d" and 1 <= int(kind[1:]) <= 6, kind
    return [c for c in CONSTRAINTS if c[2] == int(kind[1:])]


def degrees_of(kind):
    return [c[2] for c in constraints_of(kind)]


def n_columns(kind):
    return N_BASE + sum(4 if c[1] in SECURE_FORMS else 1 for c in constraints_of(kind))


# ---- the expressions over numbers: base values are one uint64 array, secure ones a list of four -------------------------------------
class _Num:
    def __init__(self, v):
        self.v = v

    @property
    def secure(self):
        return isinstance(self.v, list)

    @staticmethod
    def _lift(o):
        return o if isinstance(o, _Num) else _Num(np.uint64(int(o) % P))

    def __add__(self, o):
        o = self._lift(o)
        if self.secure and o.secure:
            return _Num([(a + b) % P for a, b in zip(self.v, o.v)])
        if not self.secure and not o.secure:
            return _Num((self.v + o.v) % P)
        e, b = (self, o) if self.secure else (o, self)
        return _Num([(e.v[0] + b.v) % P] + e.v[1:])
    __radd__ = __add__

    def __mul__(self, o):
        o = self._lift(o)
        if self.secure and o.secure:
            return _Num(qmul_rows(self.v, o.v))
        if not self.secure and not o.secure:
            return _Num(self.v * o.v % P)
        e, b = (self, o) if self.secure else (o, self)
        return _Num([x * b.v % P for x in e.v])
    __rmul__ = __mul__


class _TraceColumns:
    def __init__(self, nat):
        self.nat = nat

    def x(self, k, o=0):
        return _Num(at(self.nat[k], o))

    def one(self):
        return _Num(self.nat[COL_ONE])

    def s(self):
        return _Num(self.nat[COL_S])

    def T(self):
        return _Num([self.nat[COL_T + k] for k in range(4)])


class _RecordedColumns:
    def __init__(self, pb):
        self.pb = pb

    def x(self, k, o=0):
        return self.pb.next_trace_mask(k, (o,))[0]

    def one(self):
        return self.pb.next_trace_mask(COL_ONE)[0]

    def s(self):
        return self.pb.next_trace_mask(COL_S)[0]

    def T(self):
        return self.pb.next_secure_mask(COL_T)[0]


# ---- the trace -----------------------------------------------------------------------------------------------------------------------
def ladder_trace(kind, log, seed):
    """The columns of a valid trace of a `kind` component: (natural order, finalized to bit-reversed circle-domain order)."""
    rng = np.random.default_rng(seed)
    n = 1 << log
    nat = [rng.integers(0, P, n, dtype=np.uint64) for _ in range(N_X)]
    nat += [np.ones(n, np.uint64), rng.integers(0, 2, n, dtype=np.uint64)]
    nat += [rng.integers(0, P, n, dtype=np.uint64) for _ in range(4)]
    c = _TraceColumns(nat)
    for name, form, d, _ in constraints_of(kind):
        r = FORMS[form][1](c, d)
        assert r.secure == (form in SECURE_FORMS), name
        nat += [np.broadcast_to(v, (n,)).astype(np.uint64) for v in (r.v if r.secure else [r.v])]
    nat = [x.astype(np.uint32) for x in nat]
    assert len(nat) == n_columns(kind) and all(int(x.max()) < P for x in nat)
    return nat, [O.finalize_column(x) for x in nat]


def ladder_component(ap, kind, log, main0, bound=0):
    """The recorded component over main columns main0 .. of tree 1; nx_air_constraint_degrees gives degrees_of(kind)."""
    pb = ap.ProgramBuilder()
    c = _RecordedColumns(pb)
    col = N_BASE
    for name, form, d, _ in constraints_of(kind):
        expr = FORMS[form][1](c, d)
        if form in SECURE_FORMS:
            (r,) = pb.next_secure_mask(col)
            col += 4
        else:
            (r,) = pb.next_trace_mask(col)
            col += 1
        pb.add_constraint(r - expr)
    assert col == n_columns(kind)
    prog = pb.build()
    import nexus_zkvm_amd as nz
    assert list(nz.air_constraint_degrees(prog, col)) == degrees_of(kind), kind            # the planner sees the declared degrees
    return ap.Component(log, prog, [(1, main0 + k) for k in range(col)], log_constraint_degree_bound=bound)


def result_column(kind, j):
    """the first result column of constraint j of a `kind` component"""
    return N_BASE + sum(4 if c[1] in SECURE_FORMS else 1 for c in constraints_of(kind)[:j])


# ---- the cases: (configuration, ((kind, log_size, log_constraint_degree_bound or 0 for the configuration's), ...)) --------------------
# name -> oracle_lib.default_cfg keywords, after wide_mask_air.CONFIGS
CONFIGS = {
    "b1-lcd1": dict(pow_bits=2, log_blowup=1, log_constraint_degree=1),
    "b1-lcd2": dict(pow_bits=2, log_blowup=1, log_constraint_degree=2),
    "b2-lcd2": dict(pow_bits=2, log_blowup=2, log_constraint_degree=2),
}
SIZES = (3, 4, 5, 10)                          # the half and quarter domains need log_size >= 4: 3 is evaluated whole; 10: several blocks per kernel
SIZE_CASES = [("b1-lcd2", ((kind, log, 0),)) for log in SIZES for kind in ("d4", "d5", "mixed")]
SINGLE_DEGREE_CASES = [("b1-lcd2", ((f"d{d}", 5, 0),)) for d in (1, 2, 3)]
CONFIG_CASES = [
    ("b1-lcd1", (("low", 4, 0),)), ("b1-lcd1", (("low", 5, 0),)),
    ("b2-lcd2", (("d4", 5, 0),)), ("b2-lcd2", (("d5", 5, 0),)), ("b2-lcd2", (("mixed", 5, 0),)),      # the committed domain is the 4N one
    ("b1-lcd2", (("mixed", 5, 2), ("low", 4, 1))),                                                       # per-component bounds
]
GROUP_CASES = [
    ("b1-lcd2", (("d4", 5, 2), ("d5", 5, 2))),                         # one size: a quarter part and a full part in one group
    ("b1-lcd2", (("d4", 5, 2), ("d5", 5, 2), ("low", 6, 1))),          # beside a bound-1 component of twice the rows: the same 2^7-point domain
]
SWITCH_CASE = ("b1-lcd2", (("mixed", 5, 0),))                          # once more under "quotients.coeffs" = 0 and under "air.segment" = 200
SEGMENT_BUDGET = 200
SHARDED_CASE = ("b1-lcd2", (("mixed", 9, 0),))
PROVABLE_CASES = SIZE_CASES + SINGLE_DEGREE_CASES + CONFIG_CASES + GROUP_CASES + [SHARDED_CASE]
# above the bound: the composition does not fit the domain the bound declares, every evaluation strategy must refuse
OVER_BOUND_CASES = [("b1-lcd2", (("d6", 5, 0),)), ("b1-lcd2", (("d4", 5, 1),))]
AFTER_REFUSAL_CASE = ("b1-lcd2", (("d5", 5, 0),))


def case_id(case):
    cfg, comps = case
    return cfg + "-" + "+".join(f"{kind}.{log}" + (f".b{bound}" if bound else "") for kind, log, bound in comps)


def drive(case, seed=7):
    """The components of a case + the committed columns, after wide_mask_air.drive: mix_u64(number of components), one dummy preprocessed
    column claimed by component 0, one main tree, no interaction tree.
    Returns (run(session, commit, tamper=None) -> components, tree_logs).  tamper: (component, constraint, natural row) — that cell of the
    constraint's (first) result column is changed."""
    import nexus_zkvm_amd.air_program as ap
    _, spec = case

    def run(sess, commit, tamper=None):
        sess.mix_u64(len(spec))
        main, comps = [], []
        for i, (kind, log, bound) in enumerate(spec):
            nat, fin = ladder_trace(kind, log, seed + i)
            if tamper is not None and tamper[0] == i:
                k = result_column(kind, tamper[1])
                nat[k][tamper[2]] = (int(nat[k][tamper[2]]) + 1) % P
                fin[k] = O.finalize_column(nat[k])
            comps.append(ladder_component(ap, kind, log, len(main), bound))
            main += fin
        commit([np.zeros(1 << spec[0][1], np.uint32)])                             # a (dummy) preprocessed column
        commit(main)
        c0 = comps[0]
        comps[0] = ap.Component(c0.log_size, c0.program, c0.cols + [(0, 0)], c0.masks + [[0]], c0.log_constraint_degree_bound)
        return comps
    tree_logs = [[spec[0][1]], [log for kind, log, _ in spec for _ in range(n_columns(kind))]]
    return run, tree_logs
