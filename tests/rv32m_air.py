"""The RV32M multiply and divide chips as a device-filled statement, recorded with ProgramBuilder (nexus-zkvm_amd/air_program.py):

  fill_program()   the trace program: seeds ValueB, ValueC and the eight opcode flags; every other column of tests/rv32m_model.py's
                   layout from them — the products via pack32 / mullo32 / mulhu32, the quotient and remainder via divu32 / remu32 on
                   (absolute) values, ValueA by store_if per flag.  One call of nx_trace_program.
  constraints()    the add_constraints bodies of the five chips and of their gadgets (reference prover/src/chips/instructions/m/),
                   restated; the booleans as x (1 - x); with lookup elements, the range256 uses of the byte columns and the range8 use of
                   MulCarry1 as relation entries (chips/range_check/range256.rs:71-93, range8.rs:50).
  table()          a range table component: the preprocessed values against the multiplicity column nx_logup_multiplicities fills.

A chip writes only its own columns, so a column several chips share is the value times the sum of their flags (the flags are disjoint
bits); ValueA, which chips outside this statement write too, is stored under each flag and keeps its content on the other rows."""
import rv32m_model as M

COL, OPS = M.COL, M.OPS
LOW_OPS = ("mul", "mulh", "mulhsu", "divu", "remu", "div", "rem")          # the chips that commit the low half of the product
HIGH_OPS = ("mulhu", "mulh", "mulhsu")


def _ap():
    import nexus_zkvm_amd.air_program as ap
    return ap


# ---------------------------------------------------------------- the fill program ----------
def fill_program():
    pb = _ap().ProgramBuilder()
    load = lambda name: [pb.next_trace_mask(k)[0] for k in M.cols_of(name)]
    b, c = load("ValueB"), load("ValueC")
    f = {op: load("Is" + op.capitalize())[0] for op in OPS}
    on = lambda *ops: sum((f[o] for o in ops[1:]), f[ops[0]])
    signed_mul, unsigned_div, signed_div = on("mulh", "mulhsu"), on("divu", "remu"), on("div", "rem")

    half = lambda lo, hi: lo + hi * 256
    split = lambda h: (pb.band(h, 255), pb.shr(h, 8))

    def negate(lo, hi):
        """~v + 1 in half-words, with the carries of the increment at bits 16 and 32"""
        s0 = 0x10000 - lo
        k0 = pb.shr(s0, 16)
        s1 = 0xFFFF - hi + k0
        return pb.band(s0, 0xFFFF), pb.band(s1, 0xFFFF), k0, pb.shr(s1, 16)

    def absolute(lo, hi, sgn):
        nlo, nhi, k0, k1 = negate(lo, hi)
        return lo + sgn * (nlo - lo), hi + sgn * (nhi - hi), sgn * k0, sgn * k1

    def store_word(name, lo, hi, mask):
        for k, v in enumerate(split(lo) + split(hi)):
            pb.store(COL[name] + k, v * mask if mask is not None else v)

    b_lo, b_hi, c_lo, c_hi = half(b[0], b[1]), half(b[2], b[3]), half(c[0], c[1]), half(c[2], c[3])
    sb, sc = pb.shr(b[3], 7), pb.shr(c[3], 7)
    ab_lo, ab_hi, bb0, bb1 = absolute(b_lo, b_hi, sb)
    ac_lo, ac_hi, bc0, bc1 = absolute(c_lo, c_hi, sc)
    any_abs = signed_mul + signed_div
    store_word("ValueBAbs", ab_lo, ab_hi, any_abs)
    pb.store(COL["ValueBAbsBorrow"], bb0 * any_abs); pb.store(COL["ValueBAbsBorrow"] + 1, bb1 * any_abs)
    c_is_abs = f["mulh"] + signed_div                                  # MULHSU takes C as it is: no sign, no borrow
    sel = lambda x, y, m: y + m * (x - y)                               # m ? x : y
    vc_lo, vc_hi = sel(ac_lo, c_lo, c_is_abs), sel(ac_hi, c_hi, c_is_abs)
    store_word("ValueCAbs", vc_lo, vc_hi, any_abs)
    pb.store(COL["ValueCAbsBorrow"], bc0 * c_is_abs); pb.store(COL["ValueCAbsBorrow"] + 1, bc1 * c_is_abs)
    pb.store(COL["SgnB"], sb * any_abs)
    pb.store(COL["SgnC"], sc * c_is_abs)

    # the division on the (absolute) values: RISC-V's DIVU / REMU are total, and their zero-divisor results are what the chips commit
    dvd_lo, dvd_hi = unsigned_div * b_lo + signed_div * ab_lo, unsigned_div * b_hi + signed_div * ab_hi
    dvs_lo, dvs_hi = unsigned_div * c_lo + signed_div * ac_lo, unsigned_div * c_hi + signed_div * ac_hi
    dividend, divisor = pb.pack32(dvd_lo, dvd_hi), pb.pack32(dvs_lo, dvs_hi)
    q, r = pb.divu32(dividend, divisor), pb.remu32(dividend, divisor)
    q_lo, q_hi, r_lo, r_hi = pb.lo16(q), pb.hi16(q), pb.lo16(r), pb.hi16(r)
    any_div = unsigned_div + signed_div
    store_word("Quotient", q_lo, q_hi, any_div)
    store_word("Remainder", r_lo, r_hi, any_div)
    by_zero = pb.eq(c_lo + c_hi, 0) * any_div
    pb.store(COL["IsDivideByZero"], by_zero)
    overflow = pb.eq(b_lo, 0) * pb.eq(b_hi, 0x8000) * pb.eq(c_lo + c_hi, 2 * 0xFFFF) * signed_div
    pb.store(COL["IsOverflow"], overflow)

    # the product: MUL / MULHU of the operands, MULH / MULHSU of the absolute values, the divisions' t = quotient * divisor
    plain = on("mul", "mulhu")
    x_lo, x_hi = plain * b_lo + signed_mul * ab_lo + any_div * q_lo, plain * b_hi + signed_mul * ab_hi + any_div * q_hi
    y_own = plain + f["mulhsu"] + unsigned_div
    y_abs = f["mulh"] + signed_div
    y_lo, y_hi = y_own * c_lo + y_abs * ac_lo, y_own * c_hi + y_abs * ac_hi
    X, Y = pb.pack32(x_lo, x_hi), pb.pack32(y_lo, y_hi)
    low, high = pb.mullo32(X, Y), pb.mulhu32(X, Y)
    t_lo, t_hi, h_lo, h_hi = pb.lo16(low), pb.hi16(low), pb.lo16(high), pb.hi16(high)
    x, y = split(x_lo) + split(x_hi), split(y_lo) + split(y_hi)
    z = [x[k] * y[k] for k in range(4)]
    cross = lambda i, j: (x[i] + x[j]) * (y[i] + y[j]) - z[i] - z[j]
    low_mask, high_mask, every = on(*LOW_OPS), on(*HIGH_OPS), on(*OPS)
    p = {}
    for name, cname, (i, j), mask in (("MulP1", "MulC1", (0, 1), low_mask), ("MulP3Prime", "MulC3Prime", (0, 3), every),
                                      ("MulP3PrimePrime", "MulC3PrimePrime", (1, 2), every), ("MulP5", "MulC5", (2, 3), high_mask)):
        v = cross(i, j)
        h, cy = pb.band(v, 0xFFFF), pb.shr(v, 16)
        p[name] = split(h) + (cy,)
        pb.store(COL[name], p[name][0] * mask); pb.store(COL[name] + 1, p[name][1] * mask); pb.store(COL[cname], cy * mask)
    s0 = z[0] + p["MulP1"][0] * 256
    carry0 = pb.shr(s0, 16)
    s1 = z[1] + p["MulP1"][1] + cross(0, 2) + carry0 + (p["MulP3Prime"][0] + p["MulP3PrimePrime"][0] + p["MulP1"][2]) * 256
    carry1 = pb.shr(s1, 16)
    s2 = (z[2] + cross(1, 3) + p["MulP3Prime"][1] + p["MulP3PrimePrime"][1] + p["MulP5"][0] * 256 + carry1
          + (p["MulP3Prime"][2] + p["MulP3PrimePrime"][2]) * 256)
    carry2 = pb.shr(s2, 16)
    carry3 = pb.shr(z[3] + p["MulP5"][1] + p["MulP5"][2] * 256 + carry2, 16)
    pb.store(COL["MulCarry0"], carry0 * low_mask)
    pb.store(COL["MulCarry1"], carry1 * every)
    pb.store(COL["MulCarry2_0"], pb.band(carry2, 1) * high_mask)
    pb.store(COL["MulCarry2_1"], pb.shr(carry2, 1) * high_mask)
    pb.store(COL["MulCarry3"], carry3 * high_mask)

    # the divisions: t, the borrow of r = dividend - t at bit 16, u = divisor - r - 1 and its borrow (0 for a zero divisor)
    store_word("HelperT", t_lo, t_hi, any_div)
    pb.store(COL["RemainderBorrow"], pb.ltu(dvd_lo, t_lo) * any_div)
    not_zero = any_div - by_zero
    u0 = dvs_lo + 0xFFFF - r_lo                                         # 2^16 + (divisor_lo - r_lo - 1): bit 16 is "no borrow"
    u_borrow = 1 - pb.shr(u0, 16)
    u1 = dvs_hi + 0x10000 - r_hi - u_borrow
    store_word("HelperU", pb.band(u0, 0xFFFF), pb.band(u1, 0xFFFF), not_zero)
    pb.store(COL["HelperUBorrow"], u_borrow * not_zero)

    # MULH / MULHSU: the signed 64-bit product from |b| |c| and the signs
    store_word("ValueAAbs", t_lo, t_hi, signed_mul)
    store_word("ValueAAbsHigh", h_lo, h_hi, signed_mul)
    product_zero = pb.eq(t_lo + t_hi + h_lo + h_hi, 0)
    negative = (1 - product_zero) * (f["mulh"] * (sb + sc - sb * sc * 2) + f["mulhsu"] * sb)
    n0, n1, k0, k1 = negate(t_lo, t_hi)
    m2 = 0xFFFF - h_lo + k1
    k2 = pb.shr(m2, 16)
    m3 = 0xFFFF - h_hi + k2
    n2, n3, k3 = pb.band(m2, 0xFFFF), pb.band(m3, 0xFFFF), pb.shr(m3, 16)
    store_word("ValueALow", sel(n0, t_lo, negative), sel(n1, t_hi, negative), signed_mul)
    mulh_lo, mulh_hi = sel(n2, h_lo, negative), sel(n3, h_hi, negative)
    for k in range(2):
        pb.store(COL["ValueAAbsBorrowHigh"] + k, (k2, k3)[k] * negative)

    # DIV / REM: the signed results from the absolute quotient and remainder
    normal = signed_div - by_zero * signed_div - overflow
    qn_lo, qn_hi, qk0, qk1 = negate(q_lo, q_hi)
    flip_q = normal * (sb + sc - sb * sc * 2)
    div_lo, div_hi = sel(qn_lo, q_lo, flip_q), sel(qn_hi, q_hi, flip_q)
    rn_lo, rn_hi, rk0, rk1 = negate(r_lo, r_hi)
    rem_lo, rem_hi = sel(rn_lo, r_lo, sb), sel(rn_hi, r_hi, sb)
    div_sign, rem_sign = pb.shr(div_hi, 15), pb.shr(rem_hi, 15)
    sgn_a = negative + f["div"] * div_sign + f["rem"] * rem_sign
    pb.store(COL["SgnA"], sgn_a)
    pb.store(COL["IsAZero"], product_zero * signed_mul + f["div"] * pb.eq(div_lo + div_hi, 0) + f["rem"] * pb.eq(rem_lo + rem_hi, 0))
    for k in range(2):
        pb.store(COL["ValueAAbsBorrow"] + k, (k0, k1)[k] * negative + f["div"] * normal * div_sign * (qk0, qk1)[k] + f["rem"] * rem_sign * (rk0, rk1)[k])

    # ValueA: each chip on the rows of its own flag
    for op, (lo, hi) in (("mul", (t_lo, t_hi)), ("mulhu", (h_lo, h_hi)), ("mulh", (mulh_lo, mulh_hi)), ("mulhsu", (mulh_lo, mulh_hi)),
                         ("divu", (q_lo, q_hi)), ("remu", (r_lo, r_hi)), ("div", (div_lo, div_hi)), ("rem", (rem_lo, rem_hi))):
        for k, v in enumerate(split(lo) + split(hi)):
            pb.store_if(f[op], COL["ValueA"] + k, v)
    return pb.build_trace_program()


# ---------------------------------------------------------------- the constraints ----------
def constraints(log_size, lookups=None, first_col=0, tree=1):
    """The component.  lookups: None, or (z, alpha, claimed-sum shift, first interaction column): the range256 / range8 uses become
    relation entries and the recorder's logup constraints are added; `.builder` keeps the recorder (build_logup), `.chips` the chip of
    every constraint by ordinal: "Mul", "Mulhu", "MulhMulhsu", "DivuRemu", "DivRem", "bool", "logup"."""
    ap = _ap()
    pb = ap.ProgramBuilder()
    t = [pb.next_trace_mask(k)[0] for k in range(M.N_COLS)]
    w = lambda name: [t[k] for k in M.cols_of(name)]
    f = {op: w("Is" + op.capitalize())[0] for op in OPS}
    chips = []

    def add(chip, expr):
        chips.append(chip)
        pb.add_constraint(expr)

    half = lambda v, k: v[k] + v[k + 1] * 256
    equal = lambda chip, s, lhs, rhs: add(chip, s * (lhs - rhs))

    def absolute_32(chip, s, sgn, value, abs_value, borrow):
        equal(chip, s, (1 - sgn) * half(value, 0) + sgn * (0x10000 - half(value, 0) - borrow[0] * 0x10000), half(abs_value, 0))
        equal(chip, s, (1 - sgn) * half(value, 2) + sgn * (0xFFFF - half(value, 2) - borrow[1] * 0x10000 + borrow[0]), half(abs_value, 2))

    def absolute_64(chip, s, sgn, lo, hi, abs_lo, abs_hi, borrow_lo, borrow_hi):
        absolute_32(chip, s, sgn, lo, abs_lo, borrow_lo)
        equal(chip, s, (1 - sgn) * half(hi, 0) + sgn * (0xFFFF - half(hi, 0) - borrow_hi[0] * 0x10000 + borrow_lo[1]), half(abs_hi, 0))
        equal(chip, s, (1 - sgn) * half(hi, 2) + sgn * (0xFFFF - half(hi, 2) - borrow_hi[1] * 0x10000 + borrow_hi[0]), half(abs_hi, 2))

    zero_word = lambda chip, s, is_zero, v: equal(chip, s, is_zero * (v[0] + v[1] + v[2] + v[3]), 0)
    sign_2_to_1 = lambda chip, s, out, out_zero, a, b: equal(chip, s, out, (1 - out_zero) * (a + b - a * b * 2))
    sign_1_to_1 = lambda chip, s, out, out_zero, a: equal(chip, s, out, (1 - out_zero) * a)

    def values_equal(chip, s, a, b):
        equal(chip, s, half(a, 0), half(b, 0))
        equal(chip, s, half(a, 2), half(b, 2))

    def product(chip, s, x, y, low=None, high=None):
        """the partial products and the 16-bit assembly of x * y: low / high = the words the halves of the product must equal"""
        z = [x[k] * y[k] for k in range(4)]
        partial = lambda pname, cname, i, j: equal(chip, s, half(w(pname), 0) + w(cname)[0] * 0x10000, (x[i] + x[j]) * (y[i] + y[j]) - z[i] - z[j])
        p1, p3a, p3b, p5 = w("MulP1"), w("MulP3Prime"), w("MulP3PrimePrime"), w("MulP5")
        c1, c3a, c3b, c5 = w("MulC1")[0], w("MulC3Prime")[0], w("MulC3PrimePrime")[0], w("MulC5")[0]
        k0, k1, k20, k21, k3 = w("MulCarry0")[0], w("MulCarry1")[0], w("MulCarry2_0")[0], w("MulCarry2_1")[0], w("MulCarry3")[0]
        if low is not None:
            partial("MulP1", "MulC1", 0, 1)
        partial("MulP3Prime", "MulC3Prime", 0, 3)
        partial("MulP3PrimePrime", "MulC3PrimePrime", 1, 2)
        if high is not None:
            partial("MulP5", "MulC5", 2, 3)
        if low is not None:
            add(chip, s * (z[0] + p1[0] * 256 - k0 * 0x10000 - half(low, 0)))
            add(chip, s * (z[1] + p1[1] + (x[0] + x[2]) * (y[0] + y[2]) - z[0] - z[2] + k0 - k1 * 0x10000 + (p3a[0] + p3b[0] + c1) * 256 - half(low, 2)))
        if high is not None:
            add(chip, s * (z[2] + p3a[1] + p3b[1] + (x[1] + x[3]) * (y[1] + y[3]) - z[1] - z[3] + (p5[0] + c3b + c3a) * 256 + k1 - k20 * 0x10000 - k21 * 0x20000 - half(high, 0)))
            add(chip, s * (z[3] + p5[1] + c5 * 256 + k20 + k21 * 2 - k3 * 0x10000 - half(high, 2)))

    va, vb, vc = w("ValueA"), w("ValueB"), w("ValueC")
    # MulChip, MulhuChip
    product("Mul", f["mul"], vb, vc, low=va)
    product("Mulhu", f["mulhu"], vb, vc, high=va)
    # MulhMulhsuChip
    s = f["mulh"] + f["mulhsu"]
    ab, ac, sgn_a, sgn_b, sgn_c = w("ValueBAbs"), w("ValueCAbs"), w("SgnA")[0], w("SgnB")[0], w("SgnC")[0]
    absolute_32("MulhMulhsu", s, sgn_b, vb, ab, w("ValueBAbsBorrow"))
    absolute_32("MulhMulhsu", f["mulh"], sgn_c, vc, ac, w("ValueCAbsBorrow"))
    values_equal("MulhMulhsu", f["mulhsu"], ac, vc)
    product("MulhMulhsu", s, ab, ac, low=w("ValueAAbs"), high=w("ValueAAbsHigh"))
    a_zero = w("IsAZero")[0]
    zero_word("MulhMulhsu", s, a_zero, w("ValueAAbs"))
    zero_word("MulhMulhsu", s, a_zero, w("ValueAAbsHigh"))
    sign_2_to_1("MulhMulhsu", f["mulh"], sgn_a, a_zero, sgn_b, sgn_c)
    sign_1_to_1("MulhMulhsu", f["mulhsu"], sgn_a, a_zero, sgn_b)
    absolute_64("MulhMulhsu", s, sgn_a, w("ValueALow"), va, w("ValueAAbs"), w("ValueAAbsHigh"), w("ValueAAbsBorrow"), w("ValueAAbsBorrowHigh"))

    by_zero, overflow = w("IsDivideByZero")[0], w("IsOverflow")[0]
    quotient, remainder, helper_t, helper_u = w("Quotient"), w("Remainder"), w("HelperT"), w("HelperU")
    r_borrow, u_borrow = w("RemainderBorrow")[0], w("HelperUBorrow")[0]

    def division(chip, s, dividend, divisor):
        """t = quotient * divisor fits 32 bits, r = dividend - t, u = divisor - r - 1 unless the divisor is zero"""
        add(chip, s * ((quotient[2] + quotient[3]) * (divisor[2] + divisor[3]) + quotient[1] * divisor[3] + quotient[3] * divisor[1]))
        # the reference's order of the partial products here: P3', P3'', P1
        z = [quotient[k] * divisor[k] for k in range(4)]
        for pname, cname, (i, j) in (("MulP3Prime", "MulC3Prime", (0, 3)), ("MulP3PrimePrime", "MulC3PrimePrime", (1, 2)), ("MulP1", "MulC1", (0, 1))):
            equal(chip, s, half(w(pname), 0) + w(cname)[0] * 0x10000, (quotient[i] + quotient[j]) * (divisor[i] + divisor[j]) - z[i] - z[j])
        p1, p3a, p3b, c1, k0, k1 = w("MulP1"), w("MulP3Prime"), w("MulP3PrimePrime"), w("MulC1")[0], w("MulCarry0")[0], w("MulCarry1")[0]
        add(chip, s * (z[0] + p1[0] * 256 - k0 * 0x10000 - half(helper_t, 0)))
        add(chip, s * (z[1] + p1[1] + (quotient[0] + quotient[2]) * (divisor[0] + divisor[2]) - z[0] - z[2] + k0 - k1 * 0x10000
                       + (p3a[0] + p3b[0] + c1) * 256 - half(helper_t, 2)))
        add(chip, s * (half(dividend, 0) + r_borrow * 0x10000 - (half(helper_t, 0) + half(remainder, 0))))
        add(chip, s * (half(dividend, 2) - r_borrow - (half(helper_t, 2) + half(remainder, 2))))
        add(chip, s * (1 - by_zero) * (half(divisor, 0) + u_borrow * 0x10000 - half(remainder, 0) - 1 - half(helper_u, 0)))
        add(chip, s * (1 - by_zero) * (half(divisor, 2) - half(remainder, 2) - u_borrow - half(helper_u, 2)))

    # DivuRemuChip
    s = f["divu"] + f["remu"]
    zero_word("DivuRemu", s, by_zero, vc)
    for k in (0, 2):
        add("DivuRemu", f["divu"] * ((1 - by_zero) * half(va, k) + by_zero * 0xFFFF - half(va, k)))
    for k in (0, 2):
        add("DivuRemu", f["remu"] * ((1 - by_zero) * half(va, k) + by_zero * half(vb, k) - half(va, k)))
    values_equal("DivuRemu", f["divu"], va, quotient)
    values_equal("DivuRemu", f["remu"], va, remainder)
    division("DivuRemu", s, vb, vc)
    # DivRemChip
    s = f["div"] + f["rem"]
    zero_word("DivRem", s, by_zero, vc)
    zero_word("DivRem", s, a_zero, va)
    so = s * overflow
    equal("DivRem", so, vb[0] + vb[1] * (1 << 8) + vb[2] * (1 << 16) + vb[3] * (1 << 24), 1)            # i32::MIN mod p
    equal("DivRem", so, half(vc, 0), 0xFFFF)
    equal("DivRem", so, half(vc, 2), 0xFFFF)
    absolute_32("DivRem", s, sgn_b, vb, ab, w("ValueBAbsBorrow"))
    absolute_32("DivRem", s, sgn_c, vc, ac, w("ValueCAbsBorrow"))
    usual = 1 - by_zero - overflow
    sign_1_to_1("DivRem", f["rem"] * usual, sgn_a, a_zero, sgn_b)
    sign_2_to_1("DivRem", f["div"] * usual, sgn_a, a_zero, sgn_b, sgn_c)
    absolute_32("DivRem", f["div"] * usual, sgn_a, va, quotient, w("ValueAAbsBorrow"))
    absolute_32("DivRem", f["rem"] * (1 - by_zero), sgn_a, va, remainder, w("ValueAAbsBorrow"))
    add("DivRem", f["div"] * (usual * half(va, 0) + by_zero * 0xFFFF - half(va, 0)))
    add("DivRem", f["div"] * (usual * half(va, 2) + by_zero * 0xFFFF + overflow * 0x8000 - half(va, 2)))
    for k in (0, 2):
        add("DivRem", f["rem"] * (usual * half(va, k) + by_zero * half(vb, k) - half(va, k)))
    division("DivRem", s, ab, ac)
    # the boolean columns
    for name in M.BOOL_COLUMNS:
        for x in w(name):
            add("bool", x * (1 - x))
    cols = [(tree, first_col + k) for k in range(M.N_COLS)]
    if lookups is not None:
        z, alpha, shift, first_interaction = lookups
        rel256, rel8 = pb.relation(z[0], alpha[0], 1), pb.relation(z[1], alpha[1], 1)
        for k in byte_lookup_columns():
            pb.add_to_relation(rel256, 1, [t[k]])
        pb.add_to_relation(rel8, 1, [t[COL["MulCarry1"]]])
        pb.finalize_logup_in_pairs(M.N_COLS, shift)
        chips += ["logup"] * pb.n_logup_cols
        cols += [(2, first_interaction + k) for k in range(4 * pb.n_logup_cols)]
    comp = ap.Component(log_size, pb.build(), cols)
    comp.builder, comp.chips = pb, list(chips)
    return comp


def byte_lookup_columns():
    return [k for name in M.BYTE_COLUMNS for k in M.cols_of(name)]


def table(log_table, z, alpha, shift, cols):
    """A range table: column 0 the preprocessed values, column 1 the multiplicities, then its interaction column.  cols: the three places."""
    ap = _ap()
    pt = ap.ProgramBuilder()
    (value,), (m,) = pt.next_trace_mask(0), pt.next_trace_mask(1)
    pt.add_to_relation(pt.relation(z, alpha, 1), -m, [value])
    pt.finalize_logup(2, shift)
    comp = ap.Component(log_table, pt.build(), cols)
    comp.builder = pt
    return comp


# ---------------------------------------------------------------- the opcode table ----------
TABLE_INPUTS, TABLE_COLS = 4, 18
W_OPS = ("mullo32", "mulhu32", "divu32", "remu32")


def opcode_table():
    """The seven opcodes of the W kind: columns 0..3 hold the half-words of two 32-bit operands x, y.  Stored: the halves of
    pack32(x) (4, 5: PACK32, LO16, HI16 alone), of a pack32 whose operands are not half-words (6, 7: the truncation to 32 bits), and of
    x op y for the four integer opcodes (8..15); 16, 17: a quotient divided again, so a W result feeds a W opcode."""
    pb = _ap().ProgramBuilder()
    x_lo, x_hi, y_lo, y_hi = [pb.next_trace_mask(k)[0] for k in range(4)]
    X, Y = pb.pack32(x_lo, x_hi), pb.pack32(y_lo, y_hi)
    pb.store(4, pb.lo16(X)); pb.store(5, pb.hi16(X))
    wide = pb.pack32(x_lo * 0x7FFF + y_hi, x_hi * 3 + y_lo * 0x10001)
    pb.store(6, pb.lo16(wide)); pb.store(7, pb.hi16(wide))
    for k, name in enumerate(W_OPS):
        v = getattr(pb, name)(X, Y)
        pb.store(8 + 2 * k, pb.lo16(v)); pb.store(9 + 2 * k, pb.hi16(v))
    again = pb.remu32(pb.divu32(X, Y), pb.mullo32(Y, Y))
    pb.store(16, pb.lo16(again)); pb.store(17, pb.hi16(again))
    return pb.build_trace_program()


def opcode_table_inputs(log_size):
    """natural order: all 441 ordered pairs of E from 2^9 rows on (the other rows repeat them), a stride through them below"""
    import numpy as np
    n = 1 << log_size
    step = 1 if n >= len(M.PAIRS) else len(M.PAIRS) // n
    pairs = [M.PAIRS[(k * step) % len(M.PAIRS)] for k in range(n)]
    x, y = np.array([p[0] for p in pairs], np.uint64), np.array([p[1] for p in pairs], np.uint64)
    return [x & 0xFFFF, x >> 16, y & 0xFFFF, y >> 16]
