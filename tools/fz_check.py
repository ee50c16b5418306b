#!/usr/bin/env python3
"""tools/fz_check.py -- verifies tools/fz_check.cpp's output with big integers: the signed 13 x 30-bit Montgomery products of
csrc/fz.cuh (congruence, |value| < p, limb class, the all-limbs-zero test), its carry rounds and boundary conversions, and the
curve formulas of csrc/ecz.cuh (madd, add, dbl with their exceptional branches) against affine arithmetic.  Equality is exact,
on canonical values.  Host-only: the same headers compile for gfx950.

    g++ -O2 -std=c++17 -I mpc-jellyfish_amd/csrc tools/fz_check.cpp -o /tmp/fz_check && /tmp/fz_check 4000 | python tools/fz_check.py
The device build of the same functions: tools/fz_check_gpu.hip prints the same lines from a GPU run (python tools/fz_check.py --device).
"""
import sys

p = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
N, L = 13, 30
RP = 1 << (N * L)
RPI = pow(RP, -1, p)
R = 1 << 384
B29 = 1 << 29
val = lambda limbs: sum(int(l) << (L * i) for i, l in enumerate(limbs))
val32 = lambda words: sum(int(w) << (32 * i) for i, w in enumerate(words))


def is_m(l):                 # class M as a product returns it
    return all(-B29 <= v < B29 for v in l[:N - 1])


def is_n(l):
    return all(-B29 - 2 <= v < B29 + 2 for v in l[:N - 1])


def aff_of_pt(P):            # XYZZ limbs -> affine (true coordinates) or None
    X, Y, ZZ, ZZZ = (val(P[N * i:N * i + N]) for i in range(4))
    if ZZ % p == 0:
        assert all(v == 0 for v in P[2 * N:3 * N]), "infinity must have all-zero ZZ limbs"
        return None
    assert (ZZ * RPI) ** 3 % p == (ZZZ * RPI) ** 2 % p, "ZZ^3 != ZZZ^2"
    return (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p)


def aff_of_aff(Q):
    x, y = val(Q[:N]), val(Q[N:])
    if x % p == 0 and y % p == 0:
        assert all(v == 0 for v in Q), "affine infinity must be all-zero limbs"
        return None
    return (x * RPI % p, y * RPI % p)


def ec_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % p == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, p) % p
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, p) % p
    x = (lam * lam - a[0] - b[0]) % p
    return (x, (lam * (a[0] - x) - a[1]) % p)


def ec_neg(a):
    return None if a is None else (a[0], (-a[1]) % p)


def on_curve(a):
    return a is None or (a[1] * a[1] - a[0] ** 3 - 4) % p == 0


def check_acc(P, what):      # the accumulator invariant of ecz.cuh
    if all(v == 0 for v in P[2 * N:3 * N]):
        return
    assert is_n(P[:N]) and is_n(P[N:2 * N]) and is_m(P[2 * N:3 * N]) and is_m(P[3 * N:]), what + ": limb classes"
    assert abs(val(P[:N])) < 4 * p and abs(val(P[N:2 * N])) < 2 * p and abs(val(P[2 * N:3 * N])) < p and abs(val(P[3 * N:])) < p, what + ": value bounds"


count = {}
worst = 0.0
for line in sys.stdin:
    f = line.split()
    op, v = f[0], [int(x) for x in f[1:]]
    count[op] = count.get(op, 0) + 1
    if op in ("mul", "sqr", "mul2"):
        bounded, zero = v[0], v[1]
        v = v[2:]
        ops = [v[N * i:N * i + N] for i in range(len(v) // N)]
        r = ops[-1]
        if op == "mul":
            want = val(ops[0]) * val(ops[1])
        elif op == "sqr":
            want = val(ops[0]) ** 2
        else:
            want = val(ops[0]) * val(ops[1]) + val(ops[2]) * val(ops[3])
        assert (val(r) * RP - want) % p == 0, op + ": not congruent"
        assert is_m(r), op + ": result limbs not class M"
        if bounded:
            assert abs(val(r)) < p, (op, "range", val(r) / p)
            worst = max(worst, abs(val(r)) / p)
            assert zero == (1 if want % p == 0 else 0), op + ": fz_is_zero"
            assert zero == (1 if all(x == 0 for x in r) else 0)
    elif op == "norm":
        a, n1, n2, c = (v[N * i:N * i + N] for i in range(4))
        assert val(n1) == val(a) and val(n2) == val(a) and val(c) == val(a), "carry rounds change the value"
        assert is_n(n1) and is_n(n2) and is_m(c), "carry round classes"
    elif op == "normw":
        a, n2 = v[:N], v[N:]
        assert val(n2) == val(a) and is_n(n2), "fz_norm_wide"
    elif op == "bnd":
        img, mid, back = v[:12], v[12:12 + N], v[12 + N:]
        x = val32(img)
        assert (val(mid) * R - x * RP) % p == 0 and abs(val(mid)) < p and is_m(mid), "fz_from_boundary"
        assert val32(back) == x % p, "fz_to_boundary"
    elif op == "can":
        a, c = v[:N], v[N:]
        assert val(c) == val(a) % p and all(0 <= x < (1 << L) for x in c), "fz_canonical"
    elif op == "inv":
        a, i = v[:N], v[N:]
        x = val(a) * RPI % p
        assert val(i) * RPI % p == (pow(x, -1, p) if x else 0) and abs(val(i)) < p, "fz_inv"
    elif op == "madd":
        neg, P, Q, Rr = v[0], v[1:1 + 4 * N], v[1 + 4 * N:1 + 6 * N], v[1 + 6 * N:]
        a, b = aff_of_pt(P), aff_of_aff(Q)
        assert on_curve(a) and on_curve(b)
        assert aff_of_pt(Rr) == ec_add(a, ec_neg(b) if neg else b), "madd"
        check_acc(Rr, "madd")
    elif op == "add":
        P, Q, Rr = v[:4 * N], v[4 * N:8 * N], v[8 * N:]
        a, b = aff_of_pt(P), aff_of_pt(Q)
        assert on_curve(a) and on_curve(b)
        assert aff_of_pt(Rr) == ec_add(a, b), "add"
        check_acc(Rr, "add")
    elif op == "dbl":
        P, Rr = v[:4 * N], v[4 * N:]
        a = aff_of_pt(P)
        assert aff_of_pt(Rr) == ec_add(a, a), "dbl"
        check_acc(Rr, "dbl")
    elif op == "ptb":
        P, w = v[:4 * N], v[4 * N:]
        for i in range(4):
            assert val32(w[12 * i:12 * i + 12]) == val(P[N * i:N * i + N]) * RPI * R % p, "xyzzz_to_boundary"
    else:
        raise SystemExit("unknown line " + op)
device = "--device" in sys.argv          # tools/fz_check_gpu.hip prints the products and the curve formulas only
for need in ("mul", "sqr", "mul2", "madd", "add", "dbl") + (() if device else ("norm", "normw", "bnd", "can", "inv", "ptb")):
    assert count.get(need), "no %s cases" % need
print("fz_check: %d lines ok (%s); products of bounded operands within %.3f p" % (sum(count.values()), ", ".join("%s %d" % kv for kv in sorted(count.items())), worst))
