#!/usr/bin/env python3
"""tools/ecz_bounds.py -- worst-case bound propagation through the signed 13 x 30-bit-limb EC formulas of csrc/ecz.cuh (xyzzz_madd,
xyzzz_add, xyzzz_add_quad, xyzzz_dbl, xyzzz_dbl_affine) in exact integer arithmetic.  Every intermediate is tracked as an interval for
its limbs 0..11, a bound on |value|, and the bound on its top limb that follows from the two; every contract of csrc/fz.cuh is asserted:

  * fz_mul / fz_sqr / fz_mul2: every one of the 25 column totals (limb products + the m * p half with |m_i| <= 2^29 and p's ACTUAL
    balanced limbs + the carry from the column before) stays below 2^63 in magnitude;
  * every value stays below 2^389 in magnitude, so the top limb fits; every limb-wise sum fits int32; fz_norm's operand is within
    [-2^31, 2^31 - 2^29) (fz_norm_wide takes any int32);
  * a product's result is below p in magnitude wherever fz_is_zero is applied to it (here: everywhere);
  * the accumulator invariant -- X, Y class N with |X| < 4p, |Y| < 2p; ZZ, ZZZ class M below p -- is re-established by every formula
    from operands AT the invariant: an accumulator fed back into itself for any number of steps, and the bucket reduction's sums of sums,
    never leave it.

The tool also shows that the margins are real: the fused Y3 product is refused when its operands are merely weakly normalised
(limbs up to 2^30), and a hypothetical 13 x 30-bit product with UNSIGNED limbs is refused outright.
Run without a GPU (tests/test_ecz_bounds.py does)."""
import sys

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
N, L = 13, 30
B = 1 << (L - 1)
RP = 1 << (N * L)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def balanced(x):
    d = []
    for _ in range(N - 1):
        v = x & ((1 << L) - 1)
        if v >= B:
            v -= 1 << L
        d.append(v)
        x = (x - v) >> L
    d.append(x)
    return d


P_ABS = [abs(v) for v in balanced(P)]


class Refused(Exception):
    pass


def need(cond, msg):
    if not cond:
        raise Refused(msg)


class V:
    """limbs 0..N-2 within [lo, hi]; |value| <= val (an integer); the top limb's magnitude follows"""

    def __init__(self, lo, hi, val, name=""):
        self.lo, self.hi, self.val, self.name = lo, hi, val, name
        need(I32_MIN <= lo and hi <= I32_MAX, "%s: limb interval [%d, %d] leaves int32" % (name, lo, hi))
        need(val < 1 << (N * L - 1), "%s: |value| %.2f p reaches 2^389" % (name, val / P))
        low = max(-lo, hi) * ((1 << (L * (N - 1))) - 1) // ((1 << L) - 1)           # |sum of the low limbs| at most
        self.top = (val + low) // (1 << (L * (N - 1))) + 1
        need(self.top <= I32_MAX, "%s: top limb does not fit" % name)

    def mag(self, i):
        return self.top if i == N - 1 else max(-self.lo, self.hi)


WORST = {"col": 0, "where": ""}


def columns(pairs, name, m_limb=B):
    """column totals of sum_i x_i y_(k-i) over the operand pairs plus m * p, with the carry chain"""
    total = 0
    for k in range(2 * N - 1):
        s = 0
        for i in range(max(0, k - N + 1), min(k, N - 1) + 1):
            for x, y in pairs:
                s += x.mag(i) * y.mag(k - i)
            s += m_limb * P_ABS[k - i]
        total = s + (total + B) // (1 << L) + 1
        need(total < 1 << 63, "%s: column %d reaches %.2f * 2^58 (limit 32)" % (name, k, total / 2.0 ** 58))
        if total > WORST["col"]:
            WORST["col"], WORST["where"] = total, "%s, column %d" % (name, k)


def product(pairs, name):
    columns(pairs, name)
    val = sum(x.val * y.val for x, y in pairs) // RP + P * B // ((1 << L) - 1) + 2
    need(val < P, "%s: |result| up to %.3f p, not below p (fz_is_zero, class M)" % (name, val / P))
    return V(-B, B - 1, val, name)


def mul(a, b, name):
    return product([(a, b)], name)


def sqr(a, name):                                     # x_i * (2 x_j) once for i < j: the column magnitudes of x * x
    need(I32_MIN <= 2 * a.lo and 2 * a.hi <= I32_MAX, name + ": doubled operand")
    return product([(a, a)], name)


def mul2(x, y, u, v, name):
    return product([(x, y), (u, v)], name)


def add(a, b, name=""):
    return V(a.lo + b.lo, a.hi + b.hi, a.val + b.val, name)


def neg(a):
    return V(-a.hi, -a.lo, a.val, a.name)


def sub(a, b, name=""):
    return add(a, neg(b), name)


def norm(a, name="", wide=False):
    if not wide:
        need(a.hi + B <= I32_MAX, "%s: fz_norm's a + 2^29 overflows for limbs up to %d" % (name or a.name, a.hi))
    c_lo, c_hi = (a.lo + B) >> L, (a.hi + B) >> L
    need(abs(a.top) + max(-c_lo, c_hi) <= I32_MAX, name + ": top limb")
    return V(-B + c_lo, B - 1 + c_hi, a.val, name or a.name)


# ---- operand classes (csrc/ecz.cuh) ----
KX, KY = 4, 2


def aff_coord(name):                                  # a table entry, or its negation
    return V(-B, B, P - 1, name)


def acc_point(tag):
    n = lambda k, nm: V(-B - 2, B + 2, k * P - 1, tag + nm)
    m = lambda nm: V(-B, B, P - 1, tag + nm)
    return n(KX, ".x"), n(KY, ".y"), m(".zz"), m(".zzz")


def check_acc(x, y, zz, zzz, where):
    for v, k, lim in ((x, KX, B + 2), (y, KY, B + 2), (zz, 1, B), (zzz, 1, B)):
        need(v.val < k * P and -lim <= v.lo and v.hi <= lim, "%s: %s leaves the accumulator invariant (%.2f p, limbs [%d, %d])" % (where, v.name, v.val / P, v.lo, v.hi))


def xy3(a, b_plus_2c, q, r, y, ppp, tag):
    x3 = norm(sub(a, b_plus_2c, tag + " X3 raw"), tag + " X3", wide=True)
    d = norm(sub(q, x3, tag + " Q-X3 raw"), tag + " Q-X3")
    y3 = mul2(r, d, y, neg(ppp), tag + " Y3 = R (Q - X3) - Y1 PPP, fused")
    return x3, y3


def dbl_core(px, py, tag):
    u = norm(add(py, py), tag + " 2y")
    v = sqr(u, tag + " V")
    w = mul(u, v, tag + " W")
    s = mul(px, v, tag + " S")
    x2 = sqr(px, tag + " x^2")
    m = norm(add(add(x2, x2), x2), tag + " M", wide=True)
    mm = sqr(m, tag + " M^2")
    x3, y3 = xy3(mm, add(s, s), s, m, py, w, tag)
    return x3, y3, v, w


def dbl_affine(tag="dbl_affine"):
    x3, y3, v, w = dbl_core(aff_coord("q.x"), aff_coord("q.y"), tag)
    check_acc(x3, y3, v, w, tag)


def dbl(tag="dbl"):
    px, py, pzz, pzzz = acc_point("p")
    x3, y3, v, w = dbl_core(px, py, tag)
    check_acc(x3, y3, mul(v, pzz, tag + " ZZ3"), mul(w, pzzz, tag + " ZZZ3"), tag)


def madd(tag="madd"):
    px, py, pzz, pzzz = acc_point("p")
    qx, qy = aff_coord("q.x"), aff_coord("q.y")
    check_acc(qx, qy, V(-B, B, P - 1, "one"), V(-B, B, P - 1, "one"), tag + " (p at infinity)")
    u2 = mul(qx, pzz, tag + " U2")
    s2 = mul(qy, pzzz, tag + " S2")
    pp_ = norm(sub(u2, px), tag + " P")
    rr_ = norm(sub(s2, py), tag + " R")
    pp = sqr(pp_, tag + " PP")                         # fz_is_zero(pp), fz_is_zero(rr2): products, below p (asserted in product())
    rr2 = sqr(rr_, tag + " RR")
    dbl_affine(tag + " -> dbl_affine")
    ppp = mul(pp_, pp, tag + " PPP")
    qv = mul(px, pp, tag + " Q")
    x3, y3 = xy3(rr2, add(ppp, add(qv, qv)), qv, rr_, py, ppp, tag)
    check_acc(x3, y3, mul(pzz, pp, tag + " ZZ3"), mul(pzzz, ppp, tag + " ZZZ3"), tag)


def add_full(tag="add"):
    px, py, pzz, pzzz = acc_point("p")
    qx, qy, qzz, qzzz = acc_point("q")
    u1, u2 = mul(px, qzz, tag + " U1"), mul(qx, pzz, tag + " U2")
    s1, s2 = mul(py, qzzz, tag + " S1"), mul(qy, pzzz, tag + " S2")
    pp_ = norm(sub(u2, u1), tag + " P")
    rr_ = norm(sub(s2, s1), tag + " R")
    pp = sqr(pp_, tag + " PP")
    rr2 = sqr(rr_, tag + " RR")
    dbl(tag + " -> dbl")
    ppp = mul(pp_, pp, tag + " PPP")
    qv = mul(u1, pp, tag + " Q")
    x3, y3 = xy3(rr2, add(ppp, add(qv, qv)), qv, rr_, s1, ppp, tag)
    check_acc(x3, y3, mul(mul(pzz, qzz, tag + " zz1 zz2"), pp, tag + " ZZ3"), mul(mul(pzzz, qzzz, tag + " zzz1 zzz2"), ppp, tag + " ZZZ3"), tag)


def add_quad(tag="add_quad"):
    """all four lanes run every product: each operand is bounded by the worst coordinate a lane can hold there"""
    coord = V(-B - 2, B + 2, KX * P - 1, "any coordinate")
    p1 = mul(coord, coord, tag + " round 1")                                       # U1 | S1 | U2 | S2
    d = norm(sub(p1, p1), tag + " P | R")
    worst = lambda a, b, nm: V(min(a.lo, b.lo), max(a.hi, b.hi), max(a.val, b.val), nm)
    p2 = mul(worst(coord, d, "ca | d"), worst(coord, d, "cb | d"), tag + " round 2")
    p3 = mul(worst(d, p2, "d | u1 | p2"), p2, tag + " round 3")
    x3 = norm(sub(p2, add(p3, add(p3, p3))), tag + " X3", wide=True)
    qx = norm(sub(p3, x3), tag + " Q-X3")
    p4 = mul(worst(d, p2, "s1 | d | p2"), worst(qx, p3, "qx | ppp"), tag + " round 4")
    y3 = norm(sub(p4, p4), tag + " Y3")
    check_acc(x3, y3, p3, p4, tag)


def main():
    for f in (madd, add_full, add_quad, dbl, dbl_affine):
        f()
    print("BLS12-381 Fq on %d signed limbs of %d bits: sum |p_i| = %.2f * 2^29; every contract of fz.cuh holds in madd, add, add_quad, dbl, dbl_affine" % (N, L, sum(P_ABS) / B))
    print("  accumulator invariant |X| < %d p, |Y| < %d p, ZZ, ZZZ < p (class N / M) is closed under all five" % (KX, KY))
    print("  largest column total: %.2f * 2^58 of 32 (%s)" % (WORST["col"] / 2.0 ** 58, WORST["where"]))
    # the margins are real
    try:
        weak = V(-(1 << L), 1 << L, 5 * P, "weakly normalised")
        mul2(weak, V(-B - 2, B + 2, 4 * P, "R"), V(-B - 2, B + 2, 2 * P, "Y1"), V(-B, B, P, "PPP"), "fused Y3 with an unnormalised Q - X3")
        print("unnormalised operand ACCEPTED: the checker is broken")
        return 1
    except Refused as e:
        print("  fused Y3 with limbs up to 2^30: refused, as it must be (%s)" % e)
    try:
        u = V(0, (1 << L) - 1, P, "unsigned limbs")
        mul(u, u, "unsigned 13 x 30-bit product")
        print("unsigned 30-bit limbs ACCEPTED: the checker is broken")
        return 1
    except Refused as e:
        print("  unsigned 30-bit limbs: refused, as it must be (%s)" % e)
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except Refused as e:
        print("REFUSED: %s" % e)
        sys.exit(1)
