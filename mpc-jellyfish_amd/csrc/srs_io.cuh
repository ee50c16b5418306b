// srs_io.cuh -- G1 points of a serialized KZG setup (ark-serialize 0.4 images) <-> the SRS's boundary form, one thread per point.
//
// Records ("y is the larger" = y > q - y on canonical integers, ark's SWFlags::YIsNegative):
//   BLS12-381  compressed    48 B  x big-endian; byte 0: 0x80 compressed (must be set), 0x40 infinity, 0x20 y is the larger
//              uncompressed  96 B  x BE || y BE; byte 0: 0x80 and 0x20 must be clear, 0x40 infinity
//   BN254      compressed    32 B  x little-endian; byte 31: 0x80 y is the larger, 0x40 infinity, both = invalid
//              uncompressed  64 B  x LE (no flags) || y LE with the flags of byte 31 in byte 63 (0x80 ignored on read)
// Decoding runs the checks in the order the errors are reported (SRS_BAD_*): flags, range, square / on-curve, subgroup, infinity.
// Infinity is always refused: the library's affine SRS has no usable infinity -- (0, 0) would corrupt the mixed additions of an MSM.
// The square root is a^((q+1)/4) (q = 3 mod 4 on both curves) on the reduced-radix product of fx.cuh; G1 membership on BLS12-381 is
// the endomorphism test phi(P) = -[u^2]P of eprint 2021/1130 section 6 (u = -0xd201000000010000, phi(x, y) = (beta x, y)).
#pragma once
#include "ecx.cuh"
#include "fx.cuh"

namespace mzk {

enum SrsBad : int { SRS_BAD_FLAGS = 0, SRS_BAD_RANGE, SRS_BAD_SQUARE, SRS_BAD_CURVE, SRS_BAD_SUBGROUP, SRS_BAD_INFINITY, SRS_BAD_REASONS };

template <class X> struct SerFmt;
template <> struct SerFmt<BlsFqX> { static constexpr int BYTES = 48; static constexpr bool BE = true; };
template <> struct SerFmt<BnFqX> { static constexpr int BYTES = 32; static constexpr bool BE = false; };

// the significance-s byte (s = 0: least significant) of a field image at p
template <class X>
MZK_HD int ser_byte_pos(int s) { return SerFmt<X>::BE ? SerFmt<X>::BYTES - 1 - s : s; }

// a field image (any alignment) -> X::N little-endian 32-bit words of its integer, flag bits included
template <class X>
MZK_HD void ser_read(const uint8_t* p, uint32_t (&w)[X::N]) {
#pragma unroll
    for (int j = 0; j < X::N; j++) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) v |= (uint32_t)p[ser_byte_pos<X>(4 * j + b)] << (8 * b);
        w[j] = v;
    }
}
template <class X>
MZK_HD void ser_write(uint8_t* p, const uint32_t (&w)[X::N]) {
#pragma unroll
    for (int j = 0; j < X::N; j++)
#pragma unroll
        for (int b = 0; b < 4; b++) p[ser_byte_pos<X>(4 * j + b)] = (uint8_t)(w[j] >> (8 * b));
}
template <class X>
MZK_HD bool ser_below_modulus(const uint32_t (&w)[X::N]) {
    bool lt = false, eq = true;
#pragma unroll
    for (int j = X::N - 1; j >= 0; j--) {
        lt = lt || (eq && w[j] < X::MOD[j]);
        eq = eq && w[j] == X::MOD[j];
    }
    return lt;
}
// canonical INTEGER y (fully carried limbs, not the R'-form): y > q - y ?
template <class X>
MZK_HD bool fx_is_larger(const Fx<X>& y) {
    Fx<X> d;
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < X::XN; i++) {
        const uint32_t t = X::XP[i] - y.l[i] - b;
        b = t >> 31;
        d.l[i] = t & XMASK;
    }
    bool gt = false, eq = true;
#pragma unroll
    for (int i = X::XN - 1; i >= 0; i--) {
        gt = gt || (eq && y.l[i] > d.l[i]);
        eq = eq && y.l[i] == d.l[i];
    }
    return gt;
}
// a canonical internal value x R' -> the canonical integer x (one product)
template <class X>
MZK_HD Fx<X> fx_to_integer(const Fx<X>& a) {
    Fx<X> raw_one = Fx<X>::zero();
    raw_one.l[0] = 1;
    return fx_canonical(fx_mul(a, raw_one));
}
// q - y for a canonical y != 0, canonical (in either form: q - y R' = (-y) R')
template <class X>
MZK_HD Fx<X> fx_neg_canonical(const Fx<X>& y) {
    Fx<X> d;
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < X::XN; i++) {
        const uint32_t t = X::XP[i] - y.l[i] - b;
        b = t >> 31;
        d.l[i] = t & XMASK;
    }
    return d;
}
template <class X>
MZK_HD bool fx_eq_canonical(const Fx<X>& a, const Fx<X>& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < X::XN; i++) d |= a.l[i] ^ b.l[i];
    return d == 0;
}

// a^((p+1)/4) in the internal form: 4-bit windows from the top, as fx_inv (one call site each of fx_sqr and fx_mul; the table of
// a^0 .. a^15 is indexed at run time).  BLS12-381 Fq: 384 squarings + at most 96 products; BN254 Fq: 256 + 64.
template <class X>
MZK_HD Fx<X> fx_sqrt_candidate(const Fx<X>& a) {
    Fx<X> tab[16];
    tab[0] = Fx<X>::one();
    tab[1] = fx_mul(a, tab[0]);
#pragma unroll 1
    for (int i = 2; i < 16; i++) tab[i] = fx_mul(tab[i - 1], tab[1]);
    uint32_t e[X::N];                                            // (p + 1) / 4: p = 3 mod 4, so p + 1 carries into word 1 at most once
    uint32_t c = 1;
#pragma unroll
    for (int i = 0; i < X::N; i++) { const uint32_t t = X::MOD[i] + c; c = (c && t == 0) ? 1u : 0u; e[i] = t; }
#pragma unroll
    for (int i = 0; i < X::N; i++) e[i] = (e[i] >> 2) | (i + 1 < X::N ? e[i + 1] << 30 : 0u);
    Fx<X> acc = tab[0];
#pragma unroll 1
    for (int d = 8 * X::N - 1; d >= 0; d--) {
#pragma unroll 1
        for (int k = 0; k < 4; k++) acc = fx_sqr(acc);
        const uint32_t nib = (e[d >> 3] >> ((d & 7) * 4)) & 15u;
        if (nib) acc = fx_mul(acc, tab[nib]);
    }
    return acc;
}

// BLS12-381 G1 membership of an on-curve affine P (canonical R'-form, not infinity): phi(P) == -[u^2]P.  127 doublings and 16
// mixed additions (u^2 = 0xac45a4010001a402_0000000100000000, weight 17) -- about 1 400 products.
template <class X>
MZK_HD bool g1_in_subgroup_endo(const AffineX<X>& p) {
    constexpr uint64_t U2_HI = 0xac45a4010001a402ull, U2_LO = 0x0000000100000000ull;
    XYZZX<X> acc = XYZZX<X>::from_affine(p);
#pragma unroll 1
    for (int bit = 126; bit >= 0; bit--) {
        acc = xyzzx_dbl(acc);
        const uint64_t word = bit >= 64 ? U2_HI : U2_LO;
        if ((word >> (bit & 63)) & 1) acc = xyzzx_madd(acc, p, false);
    }
    if (acc.is_inf()) return false;
    // -[u^2]P = (X / ZZ, -Y / ZZZ) equals (beta x, y):  X - beta x ZZ = 0  and  Y + y ZZZ = 0 (mod p)
    const Fx<X> bx = fx_mul(p.x, Fx<X>::from_const(X::XENDO_BETA));                   // M
    const Fx<X> dx = fx_norm(fx_sub2(acc.x, fx_mul(bx, acc.zz)));                      // N, < (XKXY + 2) p
    const Fx<X> sy = fx_norm(fx_add(acc.y, fx_mul(p.y, acc.zzz)));                     // N, < (XKXY + 2) p
    const Fx<X> one = Fx<X>::one();
    return fx_is_zero_m(fx_mul(dx, one)) && fx_is_zero_m(fx_mul(sy, one));             // (reduced below 2p: class M)
}

// One record -> the boundary form (x*R, y*R: X::N words each) in out[0 .. 2 X::N).  Returns -1, or the first SrsBad that applies.
// ALLOW_INF (the commitments of a proof or of a verifying key, where infinity is a normal value: verifier.cuh): a point at infinity is
// not refused but FLAGGED -- SRS_INFINITY_FLAGGED is returned and out is left untouched; the SRS path keeps refusing it.
constexpr int SRS_INFINITY_FLAGGED = -2;
template <class X, bool COMPRESSED, bool VALIDATE, bool ALLOW_INF = false>
MZK_HD int srs_decode_point(const uint8_t* rec, uint32_t* out) {
    constexpr int B = SerFmt<X>::BYTES;
    constexpr bool BLS = SerFmt<X>::BE;
    uint32_t xw[X::N], yw[X::N];
    ser_read<X>(rec, xw);
    if (!COMPRESSED) ser_read<X>(rec + B, yw);
    bool inf, larger = false;
    if (BLS) {                                                   // flags: the top 3 bits of x's first (most significant) byte
        const uint32_t f = rec[0];
        if (COMPRESSED ? !(f & 0x80u) : (f & 0xA0u) != 0) return SRS_BAD_FLAGS;
        inf = f & 0x40u;
        larger = f & 0x20u;
        xw[X::N - 1] &= 0x1FFFFFFFu;
    } else {                                                     // flags: the top 2 bits of the last coordinate's last byte
        const uint32_t f = rec[COMPRESSED ? B - 1 : 2 * B - 1];
        if ((f & 0xC0u) == 0xC0u) return SRS_BAD_FLAGS;
        inf = f & 0x40u;
        larger = f & 0x80u;
        if (COMPRESSED) xw[X::N - 1] &= 0x3FFFFFFFu;
        else yw[X::N - 1] &= 0x3FFFFFFFu;
    }
    if (inf) return ALLOW_INF ? SRS_INFINITY_FLAGGED : (int)SRS_BAD_INFINITY;   // (its coordinates are not read: nothing else applies)
    if (!ser_below_modulus<X>(xw)) return SRS_BAD_RANGE;
    if (!COMPRESSED && !ser_below_modulus<X>(yw)) return SRS_BAD_RANGE;
    const Fx<X> r2 = Fx<X>::from_const(X::XR2);
    AffineX<X> p;
    p.x = fx_canonical(fx_mul(fx_unpack<X>(xw), r2));            // x R'
    const Fx<X> b = fx_canonical(fx_mul(fx_unpack<X>(X::CURVE_B), Fx<X>::from_const(X::XTO)));     // b R'
    const Fx<X> rhs = fx_canonical(fx_mul(fx_add(fx_mul(fx_sqr(p.x), p.x), b), Fx<X>::one()));   // x^3 + b (< 3p in, reduced)
    if (COMPRESSED) {
        const Fx<X> y = fx_canonical(fx_sqrt_candidate(rhs));
        if (!fx_eq_canonical(fx_canonical(fx_sqr(y)), rhs)) return SRS_BAD_SQUARE;
        p.y = fx_is_larger(fx_to_integer(y)) == larger ? y : fx_neg_canonical(y);   // (y != 0: neither curve has a point of order 2)
    } else {
        p.y = fx_canonical(fx_mul(fx_unpack<X>(yw), r2));
        if (VALIDATE && !fx_eq_canonical(fx_canonical(fx_sqr(p.y)), rhs)) return SRS_BAD_CURVE;
    }
    if constexpr (VALIDATE && BLS) {
        if (!g1_in_subgroup_endo(p)) return SRS_BAD_SUBGROUP;
    }
    if (!COMPRESSED) {                                           // (0, 0), the library's infinity, written without the flag
        uint32_t z = 0;
#pragma unroll
        for (int j = 0; j < X::N; j++) z |= xw[j] | yw[j];
        if (z == 0) return ALLOW_INF ? SRS_INFINITY_FLAGGED : (int)SRS_BAD_INFINITY;
    }
    const Fp<X> bx = fx_to_boundary<X>(p.x), by = fx_to_boundary<X>(p.y);
#pragma unroll
    for (int j = 0; j < X::N; j++) { out[j] = bx.l[j]; out[X::N + j] = by.l[j]; }
    return -1;
}

// The boundary form of one point -> its record (infinity = (0, 0) gets the infinity encoding)
template <class X, bool COMPRESSED>
MZK_HD void srs_encode_point(const uint32_t* xy, uint8_t* rec) {
    constexpr int B = SerFmt<X>::BYTES;
    constexpr bool BLS = SerFmt<X>::BE;
    const Fx<X> to = Fx<X>::from_const(X::XTO);
    const Fx<X> x = fx_to_integer(fx_mul(fx_unpack<X>(xy), to));          // x R -> x R' -> x: two products each
    const Fx<X> y = fx_to_integer(fx_mul(fx_unpack<X>(xy + X::N), to));
    uint32_t xw[X::N], yw[X::N], z = 0;
    fx_pack<X>(xw, x);
    fx_pack<X>(yw, y);
#pragma unroll
    for (int j = 0; j < X::N; j++) z |= xw[j] | yw[j];
    const bool inf = z == 0, larger = !inf && fx_is_larger(y);
    ser_write<X>(rec, xw);
    if (!COMPRESSED) ser_write<X>(rec + B, yw);
    if (BLS) rec[0] |= (uint8_t)((COMPRESSED ? 0x80u : 0u) | (inf ? 0x40u : 0u) | (COMPRESSED && larger ? 0x20u : 0u));
    else rec[COMPRESSED ? B - 1 : 2 * B - 1] |= (uint8_t)((inf ? 0x40u : 0u) | (larger ? 0x80u : 0u));
}

}  // namespace mzk
