// fz.cuh -- SIGNED reduced-radix prime-field arithmetic for gfx950: ZN limbs of 30 bits, balanced (each in about +-2^29), in
// 32-bit VGPRs; Montgomery radix R' = 2^(30*ZN).  BLS12-381 Fq: 13 limbs (390 bits, 9 bits of head-room).
//
// Why: the unsigned form (fx.cuh) needs 29-bit limbs for a column of products to fit 64 bits, so a 381-bit
// field takes 14 limbs and a Montgomery product 2 * 14^2 = 392 multiply-adds.  With limbs in [-2^29, 2^29] a product is below 2^58
// in magnitude, 13 of them plus the m*p half stay below 2^63, and the radix can be 2^30: 13 limbs, 2 * 13^2 = 338 multiply-adds
// (v_mad_i64_i32 issues at the rate of v_mad_u64_u32).  Signed values also need no multiple-of-p pad to subtract.
//
// Representation: value = sum l_i 2^(30 i), any sign, stands for itself modulo p.
//   class M : what fz_mul / fz_sqr / fz_mul2 return: limbs 0..ZN-2 in [-2^29, 2^29), the top limb whatever the value needs;
//             |value| < p when the operands meet the value bound stated on fz_mul.  A class-M value that is 0 modulo p has ALL
//             limbs zero (|value| < p leaves only 0, and balanced digits are unique).
//   class N : after fz_norm: limbs 0..ZN-2 in [-2^29 - 2, 2^29 + 2).
// The negation of a class M value has limbs in (-2^29, 2^29]: "M" below means |limb| <= 2^29.
// Column bound of a product: sum_i |x_i y_(k-i)| + sum_i |m_i| |p_(k-i)| < 2^63, where |m_i| <= 2^29 and p's balanced limbs have
// absolute sum 6.2 * 2^29: 13 |x_i||y_j| + 6.2 * 2^58 < 32 * 2^58.  tools/ecz_bounds.py proves it for every product of ecz.cuh
// from the limb bounds of the operand classes actually passed (the top limb of a value below 2^9 p is below 2^31, which matters).
#pragma once
#include "fp.cuh"

namespace mzk {

template <class Z>
struct Fz {
    static constexpr int N = Z::ZN;
    int32_t l[N];
    MZK_HD static Fz zero() {
        Fz r;
#pragma unroll
        for (int i = 0; i < N; i++) r.l[i] = 0;
        return r;
    }
    MZK_HD static Fz from_const(const int32_t (&c)[Z::ZN]) {
        Fz r;
#pragma unroll
        for (int i = 0; i < N; i++) r.l[i] = c[i];
        return r;
    }
    MZK_HD static Fz one() { return from_const(Z::ZONE); }
};

// the low 30 bits of v as a signed number in [-2^29, 2^29): one v_bfe_i32
MZK_HD int32_t fz_sext(uint32_t v) { return (int32_t)(v << 2) >> 2; }
// p's balanced limbs as values the compiler cannot see through (fs.cuh, fs_neg_p_limb: limb 0 is -21845 = -(2^16 - 1) / 3, and clang
// turns m * (small constant of special shape) into 64-bit shift / subtract sequences where one v_mad_i64_i32 does)
template <class Z>
MZK_HD int32_t fz_p_limb(int i) {
    int32_t v = Z::ZP[i];
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(v));
#endif
    return v;
}

// x*y/R' mod p.  Requires every column sum below 2^63 (header) and |x||y| < R' p / 2: then the result is class M with
// |value| <= |x||y|/R' + p (1/2 + 2^-30) -- below p for |x| <= A p, |y| <= B p with A B < 2^8.
template <class Z>
MZK_HD Fz<Z> fz_mul(const Fz<Z>& x, const Fz<Z>& y) {
    constexpr int N = Z::ZN;
    int32_t m[N], pl[N];
#pragma unroll
    for (int i = 0; i < N; i++) pl[i] = fz_p_limb<Z>(i);
    Fz<Z> t;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) acc += (int64_t)x.l[i] * y.l[k - i];
#pragma unroll
        for (int i = 0; i < k; i++) acc += (int64_t)m[i] * pl[k - i];
        m[k] = fz_sext((uint32_t)acc * Z::ZINV);
        acc += (int64_t)m[k] * pl[0];
        acc >>= Z::ZL;                                               // exact: the low 30 bits are zero
    }
#pragma unroll
    for (int k = N; k < 2 * N - 1; k++) {
#pragma unroll
        for (int i = k - N + 1; i < N; i++) {
            acc += (int64_t)x.l[i] * y.l[k - i];
            acc += (int64_t)m[i] * pl[k - i];
        }
        t.l[k - N] = fz_sext((uint32_t)acc);
        acc = (acc + (1 << (Z::ZL - 1))) >> Z::ZL;                   // (acc - digit) / 2^30
    }
    t.l[N - 1] = (int32_t)acc;
    return t;
}
// (x*y + u*v)/R' mod p with ONE Montgomery reduction: 3 N^2 multiply-adds instead of 4 N^2.  Column sums: twice those of a product
// plus one m*p half -- with all four operands at |limb| <= 2^29 + 2 that is 26 * 2^58 + 6.2 * 2^58 > 2^63 at face value, and holds only
// because the terms that involve a top limb are small (tools/ecz_bounds.py: 30.2 * 2^58 for the operands ecz.cuh passes).
// |value| <= (|x||y| + |u||v|)/R' + p (1/2 + 2^-30).
template <class Z>
MZK_HD Fz<Z> fz_mul2(const Fz<Z>& x, const Fz<Z>& y, const Fz<Z>& u, const Fz<Z>& v) {
    constexpr int N = Z::ZN;
    int32_t m[N], pl[N];
#pragma unroll
    for (int i = 0; i < N; i++) pl[i] = fz_p_limb<Z>(i);
    Fz<Z> t;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) {
            acc += (int64_t)x.l[i] * y.l[k - i];
            acc += (int64_t)u.l[i] * v.l[k - i];
        }
#pragma unroll
        for (int i = 0; i < k; i++) acc += (int64_t)m[i] * pl[k - i];
        m[k] = fz_sext((uint32_t)acc * Z::ZINV);
        acc += (int64_t)m[k] * pl[0];
        acc >>= Z::ZL;
    }
#pragma unroll
    for (int k = N; k < 2 * N - 1; k++) {
#pragma unroll
        for (int i = k - N + 1; i < N; i++) {
            acc += (int64_t)x.l[i] * y.l[k - i];
            acc += (int64_t)u.l[i] * v.l[k - i];
            acc += (int64_t)m[i] * pl[k - i];
        }
        t.l[k - N] = fz_sext((uint32_t)acc);
        acc = (acc + (1 << (Z::ZL - 1))) >> Z::ZL;
    }
    t.l[N - 1] = (int32_t)acc;
    return t;
}
// x^2/R': the off-diagonal products are taken once against the doubled operand (|limb| doubles, the number of terms halves: the
// column bound is that of fz_mul(x, x)), N(N+1)/2 multiply-adds for the x*x half.  Same contract as fz_mul.
template <class Z>
MZK_HD Fz<Z> fz_sqr(const Fz<Z>& x) {
    constexpr int N = Z::ZN;
    int32_t m[N], pl[N], x2[N];
#pragma unroll
    for (int i = 0; i < N; i++) { pl[i] = fz_p_limb<Z>(i); x2[i] = x.l[i] * 2; }
    Fz<Z> t;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
#pragma unroll
        for (int i = 0; 2 * i < k; i++) acc += (int64_t)x.l[i] * x2[k - i];
        if (k % 2 == 0) acc += (int64_t)x.l[k / 2] * x.l[k / 2];
#pragma unroll
        for (int i = 0; i < k; i++) acc += (int64_t)m[i] * pl[k - i];
        m[k] = fz_sext((uint32_t)acc * Z::ZINV);
        acc += (int64_t)m[k] * pl[0];
        acc >>= Z::ZL;
    }
#pragma unroll
    for (int k = N; k < 2 * N - 1; k++) {
#pragma unroll
        for (int i = k - N + 1; 2 * i < k; i++) acc += (int64_t)x.l[i] * x2[k - i];
        if (k % 2 == 0) acc += (int64_t)x.l[k / 2] * x.l[k / 2];
#pragma unroll
        for (int i = k - N + 1; i < N; i++) acc += (int64_t)m[i] * pl[k - i];
        t.l[k - N] = fz_sext((uint32_t)acc);
        acc = (acc + (1 << (Z::ZL - 1))) >> Z::ZL;
    }
    t.l[N - 1] = (int32_t)acc;
    return t;
}

// limb-wise, no carries: limb and value bounds add.  The sums must fit int32.
template <class Z>
MZK_HD Fz<Z> fz_add(const Fz<Z>& a, const Fz<Z>& b) {
    Fz<Z> r;
#pragma unroll
    for (int i = 0; i < Z::ZN; i++) r.l[i] = a.l[i] + b.l[i];
    return r;
}
template <class Z>
MZK_HD Fz<Z> fz_sub(const Fz<Z>& a, const Fz<Z>& b) {
    Fz<Z> r;
#pragma unroll
    for (int i = 0; i < Z::ZN; i++) r.l[i] = a.l[i] - b.l[i];
    return r;
}
template <class Z>
MZK_HD Fz<Z> fz_neg(const Fz<Z>& a) {                                // limbs > -2^31
    Fz<Z> r;
#pragma unroll
    for (int i = 0; i < Z::ZN; i++) r.l[i] = -a.l[i];
    return r;
}

// one round of signed carries, all limbs at once: limbs in [-2^31, 2^31 - 2^29) in (|limb| <= 3 * 2^29 - 1), class N out -- limbs
// 0..ZN-2 in [-2^29 - 2, 2^29 + 2), the top limb keeps everything.  The value is unchanged.
template <class Z>
MZK_HD Fz<Z> fz_norm(const Fz<Z>& a) {
    constexpr int N = Z::ZN, L = Z::ZL;
    Fz<Z> r;
    r.l[0] = fz_sext((uint32_t)a.l[0]);
#pragma unroll
    for (int i = 1; i < N - 1; i++) r.l[i] = fz_sext((uint32_t)a.l[i]) + ((a.l[i - 1] + (1 << (L - 1))) >> L);
    r.l[N - 1] = a.l[N - 1] + ((a.l[N - 2] + (1 << (L - 1))) >> L);
    return r;
}
// the same for ANY int32 limbs (one more instruction per limb: the rounding carry without the overflowing addition)
template <class Z>
MZK_HD Fz<Z> fz_norm_wide(const Fz<Z>& a) {
    constexpr int N = Z::ZN, L = Z::ZL;
    Fz<Z> r;
    r.l[0] = fz_sext((uint32_t)a.l[0]);
#pragma unroll
    for (int i = 1; i < N - 1; i++) r.l[i] = fz_sext((uint32_t)a.l[i]) + (((a.l[i - 1] >> (L - 1)) + 1) >> 1);
    r.l[N - 1] = a.l[N - 1] + (((a.l[N - 2] >> (L - 1)) + 1) >> 1);
    return r;
}
// full carry propagation to balanced digits: limbs 0..ZN-2 in [-2^29, 2^29) (|limbs| < 2^31 - 2^29 in, |value| < 2^389)
template <class Z>
MZK_HD Fz<Z> fz_carry(const Fz<Z>& a) {
    constexpr int N = Z::ZN, L = Z::ZL;
    Fz<Z> r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        const int32_t t = a.l[i] + c;
        r.l[i] = fz_sext((uint32_t)t);
        c = ((t >> (L - 1)) + 1) >> 1;                               // (t - digit) / 2^30 without an overflowing step
    }
    r.l[N - 1] = a.l[N - 1] + c;
    return r;
}
// value == 0 (mod p) for a class-M value with |value| < p (what fz_mul returns): all limbs zero is the whole test
template <class Z>
MZK_HD bool fz_is_zero(const Fz<Z>& a) {
    int32_t z = 0;
#pragma unroll
    for (int i = 0; i < Z::ZN; i++) z |= a.l[i];
    return z == 0;
}
// |value| < p, |limbs| < 2^31 - 2^29  ->  the representative in [0, p) with limbs in [0, 2^30)
template <class Z>
MZK_HD Fz<Z> fz_canonical(const Fz<Z>& a) {
    constexpr int N = Z::ZN, L = Z::ZL;
    constexpr int32_t MASK = (1 << L) - 1;
    Fz<Z> r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        const int32_t t = a.l[i] + c;
        r.l[i] = t & MASK;
        c = t >> L;
    }
    r.l[N - 1] = a.l[N - 1] + c;                                     // its sign is the value's
    const bool negative = r.l[N - 1] < 0;
    Fz<Z> s;
    c = 0;
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        const int32_t t = r.l[i] + Z::ZPU[i] + c;
        s.l[i] = t & MASK;
        c = t >> L;
    }
    s.l[N - 1] = r.l[N - 1] + Z::ZPU[N - 1] + c;
#pragma unroll
    for (int i = 0; i < N; i++) r.l[i] = negative ? s.l[i] : r.l[i];
    return r;
}

// boundary image (Z::N little-endian 32-bit words, value < 2^(30*ZN - 1)) -> balanced 30-bit limbs
template <class Z>
MZK_HD Fz<Z> fz_unpack(const uint32_t* w) {
    constexpr int N = Z::ZN, W = Z::N, L = Z::ZL;
    Fz<Z> r;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const int bit = L * i, wi = bit >> 5, s = bit & 31;
        uint32_t v = wi < W ? (w[wi] >> s) : 0u;
        if (s > 32 - L && wi + 1 < W) v |= w[wi + 1] << (32 - s);
        r.l[i] = (int32_t)(v & ((1u << L) - 1));
    }
    return fz_carry(r);
}
// limbs in [0, 2^30), value < 2^(32*Z::N) -> boundary image
template <class Z>
MZK_HD void fz_pack(uint32_t* w, const Fz<Z>& a) {
    constexpr int N = Z::ZN, W = Z::N, L = Z::ZL;
#pragma unroll
    for (int j = 0; j < W; j++) {
        const int bit = 32 * j, i0 = bit / L, o = bit - L * i0;
        uint32_t v = i0 < N ? (uint32_t)a.l[i0] >> o : 0u;
        if (i0 + 1 < N) v |= (uint32_t)a.l[i0 + 1] << (L - o);
        if (2 * L - o < 32 && i0 + 2 < N) v |= (uint32_t)a.l[i0 + 2] << (2 * L - o);
        w[j] = v;
    }
}

// boundary <-> internal
template <class Z>
MZK_HD Fz<Z> fz_from_boundary(const Fp<Z>& a) {                // x*R (packed, any value < 2^384) -> x*R', class M, |value| < p
    return fz_mul(fz_unpack<Z>(a.l), Fz<Z>::from_const(Z::ZTO));
}
template <class Z>
MZK_HD Fp<Z> fz_to_boundary(const Fz<Z>& a) {                  // lazy x*R' (any operand fz_mul accepts) -> x*R canonical, packed
    Fp<Z> r;
    fz_pack<Z>(r.l, fz_canonical(fz_mul(a, Fz<Z>::from_const(Z::ZFROM))));
    return r;
}

// 1/a in the internal form (a R' -> a^-1 R'), fz_inv(0) = 0: a^(p-2) with 4-bit windows taken from the top, as fx_inv (fx.cuh).
// a: any operand fz_mul accepts; class M out.
template <class Z>
MZK_HD Fz<Z> fz_inv(const Fz<Z>& a) {
    Fz<Z> tab[16];
    tab[0] = Fz<Z>::one();
    tab[1] = fz_mul(a, tab[0]);
#pragma unroll 1
    for (int i = 2; i < 16; i++) tab[i] = fz_mul(tab[i - 1], tab[1]);
    uint32_t e[Z::N];                                                // p - 2
#pragma unroll
    for (int i = 0; i < Z::N; i++) e[i] = Z::MOD[i];
    uint32_t borrow = e[0] < 2 ? 1u : 0u;
    e[0] -= 2;
#pragma unroll
    for (int i = 1; i < Z::N; i++) { const uint32_t t = e[i]; e[i] = t - borrow; borrow = (borrow && t == 0) ? 1u : 0u; }
    Fz<Z> acc = tab[0];
#pragma unroll 1
    for (int d = 8 * Z::N - 1; d >= 0; d--) {
#pragma unroll 1
        for (int k = 0; k < 4; k++) acc = fz_sqr(acc);
        const uint32_t nib = (e[d >> 3] >> ((d & 7) * 4)) & 15u;
        if (nib) acc = fz_mul(acc, tab[nib]);
    }
    return acc;
}

}  // namespace mzk
