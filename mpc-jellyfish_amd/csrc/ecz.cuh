// ecz.cuh -- G1 bucket arithmetic on the signed 30-bit-limb field (fz.cuh): BLS12-381 Fq on 13 limbs.  The formulas and their
// exceptional branches are those of ecx.cuh (EFD madd-2008-s / add-2008-s / dbl-2008-s-1 / mdbl-2008-s-1); what differs is the
// bookkeeping: a signed a - b needs no multiple-of-p pad, a product returns |value| < p whatever (small) multiples of p went in, and
// "== 0 mod p" is "all limbs zero".  This is a file of its own rather than ecx.cuh templated on the field operations, so that BN254's
// instantiation of ecx.cuh compiles from unchanged source.
//
// Limb classes (fz.cuh):  M = |limb| <= 2^29 (a product, or its negation),  N = |limb| <= 2^29 + 2 (after fz_norm); the top limb is
// bounded by the value.  Invariant of an accumulator: X, Y in N with |X| < 5p, |Y| < 3p; ZZ, ZZZ in M, |value| < p; infinity <=> ZZ == 0
// (all limbs).  An affine point: x, y in M with |value| < p; (0, 0) = infinity.
// tools/ecz_bounds.py walks every line below with these classes: column sums below 2^63, values below 2^389, and |value| < p wherever
// fz_is_zero is applied.
#pragma once
#include "ecx.cuh"
#include "fz.cuh"

namespace mzk {

template <class Z>
struct AffineZ {               // x, y class M, |value| < p, in R'-form; (0,0) = infinity
    Fz<Z> x, y;
    MZK_HD bool is_inf() const {
        int32_t a = 0;
#pragma unroll
        for (int i = 0; i < Z::ZN; i++) a |= x.l[i] | y.l[i];
        return a == 0;
    }
};

template <class Z>
struct XYZZZ {
    Fz<Z> x, y, zz, zzz;
    MZK_HD bool is_inf() const { return fz_is_zero(zz); }
    MZK_HD static XYZZZ inf() {
        XYZZZ r;
        r.x = Fz<Z>::one(); r.y = Fz<Z>::one(); r.zz = Fz<Z>::zero(); r.zzz = Fz<Z>::zero();
        return r;
    }
    MZK_HD static XYZZZ from_affine(const AffineZ<Z>& p) {
        if (p.is_inf()) return inf();
        XYZZZ r;
        r.x = p.x; r.y = p.y; r.zz = Fz<Z>::one(); r.zzz = Fz<Z>::one();
        return r;
    }
};

// X3 = a - b - 2c and Y3 = r (q - X3) - y ppp in one reduction: the tail shared by every formula below
// a, b, c, q in M (c == q in the additions; a = M^2, b = 0 in the doublings); r, y in N; ppp in M
template <class Z>
MZK_HD void ecz_xy3(Fz<Z>& x3, Fz<Z>& y3, const Fz<Z>& a, const Fz<Z>& b_plus_2c, const Fz<Z>& q, const Fz<Z>& r, const Fz<Z>& y, const Fz<Z>& ppp) {
    x3 = fz_norm_wide(fz_sub(a, b_plus_2c));                                // |limb| <= 4 * 2^29 in: N, |value| < 4p
    const Fz<Z> d = fz_norm(fz_sub(q, x3));                                 // N, < 5p
    y3 = fz_mul2(r, d, y, fz_neg(ppp));                                     // M, < p
}

// 2*P for affine P (mdbl-2008-s-1); cold path
template <class Z>
MZK_HD XYZZZ<Z> xyzzz_dbl_affine(const AffineZ<Z>& p) {
    XYZZZ<Z> r;
    const Fz<Z> u = fz_norm(fz_add(p.y, p.y));                              // 2y, N
    const Fz<Z> v = fz_sqr(u);                                              // M
    const Fz<Z> w = fz_mul(u, v);                                           // M
    const Fz<Z> s = fz_mul(p.x, v);                                         // M
    const Fz<Z> x2 = fz_sqr(p.x);                                           // M
    const Fz<Z> m = fz_norm_wide(fz_add(fz_add(x2, x2), x2));               // 3x^2, N, < 3p
    const Fz<Z> mm = fz_sqr(m);                                             // M
    ecz_xy3<Z>(r.x, r.y, mm, fz_add(s, s), s, m, p.y, w);
    r.zz = v;
    r.zzz = w;
    return r;
}

// 2*P (dbl-2008-s-1); cold path
template <class Z>
MZK_HD XYZZZ<Z> xyzzz_dbl(const XYZZZ<Z>& p) {
    if (p.is_inf()) return p;
    XYZZZ<Z> r;
    const Fz<Z> u = fz_norm(fz_add(p.y, p.y));                              // N
    const Fz<Z> v = fz_sqr(u);
    const Fz<Z> w = fz_mul(u, v);
    const Fz<Z> s = fz_mul(p.x, v);
    const Fz<Z> x2 = fz_sqr(p.x);
    const Fz<Z> m = fz_norm_wide(fz_add(fz_add(x2, x2), x2));
    const Fz<Z> mm = fz_sqr(m);
    ecz_xy3<Z>(r.x, r.y, mm, fz_add(s, s), s, m, p.y, w);
    r.zz = fz_mul(v, p.zz);
    r.zzz = fz_mul(w, p.zzz);
    return r;
}

// P +- Q, Q affine; `negate` adds -Q.  10 products -- the two of Y3 share one Montgomery reduction (fz_mul2) --, 4 carry rounds.
template <class Z>
MZK_HD XYZZZ<Z> xyzzz_madd(const XYZZZ<Z>& p, const AffineZ<Z>& q, bool negate) {
    if (q.is_inf()) return p;
    const Fz<Z> qy = negate ? fz_neg(q.y) : q.y;                            // M
    if (p.is_inf()) {
        XYZZZ<Z> r;
        r.x = q.x; r.y = qy; r.zz = Fz<Z>::one(); r.zzz = Fz<Z>::one();
        return r;
    }
    const Fz<Z> u2 = fz_mul(q.x, p.zz);                                     // M
    const Fz<Z> s2 = fz_mul(qy, p.zzz);                                     // M
    const Fz<Z> pp_ = fz_norm(fz_sub(u2, p.x));                             // U2 - X1: N, < 6p
    const Fz<Z> rr_ = fz_norm(fz_sub(s2, p.y));                             // S2 - Y1: N, < 4p
    const Fz<Z> pp = fz_sqr(pp_);                                           // M, < p
    const Fz<Z> rr2 = fz_sqr(rr_);                                          // M, < p
    if (fz_is_zero(pp)) {                                                   // U2 == X1 (mod p)
        if (fz_is_zero(rr2)) {                                              // same point: double it
            AffineZ<Z> qq;
            qq.x = q.x;
            qq.y = qy;
            return xyzzz_dbl_affine(qq);
        }
        return XYZZZ<Z>::inf();                                             // P = -Q
    }
    XYZZZ<Z> r;
    const Fz<Z> ppp = fz_mul(pp_, pp);                                      // M
    const Fz<Z> qv = fz_mul(p.x, pp);                                       // M
    ecz_xy3<Z>(r.x, r.y, rr2, fz_add(ppp, fz_add(qv, qv)), qv, rr_, p.y, ppp);   // R^2 - PPP - 2Q;  R (Q - X3) - Y1 PPP
    r.zz = fz_mul(p.zz, pp);                                                // M
    r.zzz = fz_mul(p.zzz, ppp);                                             // M
    return r;
}

// P + Q, both accumulators.  14 products (two of them fused into one reduction).
template <class Z>
MZK_HD XYZZZ<Z> xyzzz_add(const XYZZZ<Z>& p, const XYZZZ<Z>& q) {
    if (q.is_inf()) return p;
    if (p.is_inf()) return q;
    const Fz<Z> u1 = fz_mul(p.x, q.zz), u2 = fz_mul(q.x, p.zz);             // M
    const Fz<Z> s1 = fz_mul(p.y, q.zzz), s2 = fz_mul(q.y, p.zzz);           // M
    const Fz<Z> pp_ = fz_norm(fz_sub(u2, u1));                              // N, < 2p
    const Fz<Z> rr_ = fz_norm(fz_sub(s2, s1));                              // N
    const Fz<Z> pp = fz_sqr(pp_);
    const Fz<Z> rr2 = fz_sqr(rr_);
    if (fz_is_zero(pp)) {
        if (fz_is_zero(rr2)) return xyzzz_dbl(p);
        return XYZZZ<Z>::inf();
    }
    XYZZZ<Z> r;
    const Fz<Z> ppp = fz_mul(pp_, pp);
    const Fz<Z> qv = fz_mul(u1, pp);
    ecz_xy3<Z>(r.x, r.y, rr2, fz_add(ppp, fz_add(qv, qv)), qv, rr_, s1, ppp);
    r.zz = fz_mul(fz_mul(p.zz, q.zz), pp);
    r.zzz = fz_mul(fz_mul(p.zzz, q.zzz), ppp);
    return r;
}

#if defined(__HIPCC__)
// ---- one addition on FOUR lanes: ecx.cuh's xyzzx_add_quad (the round table is there) on the signed field ----------------------------
// Same operations and operand classes as xyzzz_add except Y3, which is the difference of two products held by different lanes
// (class N, < 2p) instead of one fused product.
template <int CTRL, class Z>
__device__ __forceinline__ Fz<Z> fz_quad_perm(const Fz<Z>& a) {
    Fz<Z> r;
#pragma unroll
    for (int i = 0; i < Z::ZN; i++) {
        r.l[i] = __builtin_amdgcn_update_dpp(0, a.l[i], CTRL, 0xF, 0xF, true);
        // keep the permute a v_mov_b32_dpp of its own.  Signed limbs subtract without a pad, so a permuted SUBTRAHEND reaches a
        // plain v_sub, which the compiler folds into v_subrev_u32_dpp -- and on the device that form returned the NEGATED
        // difference (Y3 of every quad addition: tools/fz_check_gpu.hip).  ecx.cuh never meets it: there a permuted value is
        // subtracted from a pad first.  The instruction count is that of ecx.cuh's permutes.
        asm("" : "+v"(r.l[i]));
    }
    return r;
}
template <class Z>
__device__ __forceinline__ Fz<Z> fz_sel(bool c, const Fz<Z>& a, const Fz<Z>& b) {
    Fz<Z> r;
#pragma unroll
    for (int i = 0; i < Z::ZN; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}

// ca, cb: coordinate `role` of the accumulators a and b; returns coordinate `role` of a + b.  The four lanes of a quad must all be active.
template <class Z>
__device__ __forceinline__ Fz<Z> xyzzz_add_quad(const Fz<Z>& ca, const Fz<Z>& cb, int role) {
    const bool r0 = role == 0, r1 = role == 1, hi = role >= 2;
    int special = (role == 2 && (fz_is_zero(ca) || fz_is_zero(cb))) ? 1 : 0;   // an operand at infinity (zz == 0)
    const Fz<Z> p1 = fz_mul(ca, fz_quad_perm<QP_SWAP2>(cb));                    // U1 | S1 | U2 | S2
    const Fz<Z> d = fz_norm(fz_sub(fz_quad_perm<QP_SWAP2>(p1), p1));            // P | R | -P | -R: N, < 2p
    const Fz<Z> p2 = fz_mul(fz_sel(hi, ca, d), fz_sel(hi, cb, d));              // PP | RR | zz1 zz2 | zzz1 zzz2
    if (r0 && fz_is_zero(p2)) special = 1;                                      // U2 == U1: the same point or inverse points
    special |= __builtin_amdgcn_update_dpp(0, special, QP_SWAP1, 0xF, 0xF, true);
    special |= __builtin_amdgcn_update_dpp(0, special, QP_SWAP2, 0xF, 0xF, true);
    if (special) {                                                              // (quad-uniform) every lane adds the whole points
        XYZZZ<Z> a, b;
        a.x = fz_quad_perm<QP_L0>(ca); a.y = fz_quad_perm<QP_L1>(ca); a.zz = fz_quad_perm<QP_L2>(ca); a.zzz = fz_quad_perm<QP_L3>(ca);
        b.x = fz_quad_perm<QP_L0>(cb); b.y = fz_quad_perm<QP_L1>(cb); b.zz = fz_quad_perm<QP_L2>(cb); b.zzz = fz_quad_perm<QP_L3>(cb);
        const XYZZZ<Z> r = xyzzz_add(a, b);
        return fz_sel(hi, fz_sel(role == 2, r.zz, r.zzz), fz_sel(r0, r.x, r.y));
    }
    const Fz<Z> pp = fz_quad_perm<QP_L0>(p2);
    const Fz<Z> u1 = fz_quad_perm<QP_L0>(p1);
    const Fz<Z> p3 = fz_mul(fz_sel(r0, d, fz_sel(r1, u1, p2)), pp);             // PPP | Q | ZZ3 | -
    const Fz<Z> ppp = fz_quad_perm<QP_L0>(p3);
    const Fz<Z> x3 = fz_norm_wide(fz_sub(p2, fz_add(ppp, fz_add(p3, p3))));     // L1: RR - PPP - 2Q: N, < 4p
    const Fz<Z> qx = fz_norm(fz_sub(p3, x3));                                   // L1: Q - X3: N, < 5p
    const Fz<Z> s1 = fz_quad_perm<QP_L1>(p1);
    const Fz<Z> p4 = fz_mul(fz_sel(r0, s1, fz_sel(r1, d, p2)), fz_sel(r1, qx, ppp));             // S1 PPP | R (Q - X3) | - | ZZZ3
    const Fz<Z> y3 = fz_norm(fz_sub(p4, fz_quad_perm<QP_L0>(p4)));              // L1: N, < 2p
    const Fz<Z> x3_0 = fz_quad_perm<QP_L1>(x3);
    return fz_sel(hi, fz_sel(role == 2, p3, p4), fz_sel(r0, x3_0, y3));
}
#endif

template <class Z>
MZK_HD XYZZ<Fp<Z>> xyzzz_to_boundary(const XYZZZ<Z>& p) {
    XYZZ<Fp<Z>> r;
    if (p.is_inf()) return XYZZ<Fp<Z>>::inf();
    r.x = fz_to_boundary<Z>(p.x); r.y = fz_to_boundary<Z>(p.y);
    r.zz = fz_to_boundary<Z>(p.zz); r.zzz = fz_to_boundary<Z>(p.zzz);
    return r;
}

}  // namespace mzk
