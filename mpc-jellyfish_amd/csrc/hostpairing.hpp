// hostpairing.hpp -- host-only optimal ate pairings on BLS12-381 and BN254, over hostfp.hpp / hostinv.hpp: what the verifier's final
// check e(A, beta_h) e(-B, h) = 1 runs (two Miller loops and one final exponentiation per batch, whatever the batch size), with the G2
// arithmetic and the G2 records of an OpenKey.
//
// Towers: Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v); xi = 1 + u (BLS12-381), 9 + u (BN254).
// G2 is the order-r subgroup of the sextic twist E'/Fq2: y^2 = x^3 + b xi (BLS12-381: (x, y) -> (x / w^2, y / w^3) onto E) resp.
// y^2 = x^3 + b / xi (BN254: (x, y) -> (x w^2, y w^3)).
// Miller loop: affine coordinates on the twist, one Fq2 inversion per step (~5 us each by division steps; ~70 steps), plain
// double-and-add over |x| = 0xd201000000010000 resp. 6x + 2 = 0x19d797039be763ba8.  A line through T with twist slope l, evaluated at
// P = (xP, yP) in G1, is up to a factor of a proper subfield (which the final exponentiation sends to 1)
//     BN254      yP  -  l xP w  +  (l xT - yT) w^3
//     BLS12-381  (l xT - yT)  -  l xP w^2  +  yP w^3
// BN254 ends with the lines through pi(Q) and -pi^2(Q); BLS12-381's x is negative, so its Miller value is conjugated (as ark-ec does).
// Final exponentiation by the definition's exponent (q^12 - 1) / r: f^(q^6 - 1) by a conjugate and an inversion, ^(q^2 + 1) by a
// Frobenius, then the power (q^4 - q^2 + 1) / r with a 4-bit window.
// Product code: not shared with oracle/.
#pragma once
#include <cstdint>
#include <cstring>

#include "hostfp.hpp"

namespace mzk {
namespace hpair {

// ---- curves ---------------------------------------------------------------------------------------------------------------------------
struct Bls12 {
    using P = BlsFq;
    static constexpr int N = 6;                         // 64-bit limbs of Fq
    static constexpr int FB = 48;                       // bytes of an Fq record
    static constexpr bool BE = true;                    // records: big-endian, c1 first, flags in byte 0
    static constexpr int XI0 = 1;                       // xi = XI0 + u
    static constexpr bool TWIST_MUL = true;             // b' = b xi
    static constexpr bool BN_LINES = false, NEG_X = true;
    static constexpr int ATE_BITS = 64;
    static constexpr uint64_t ATE[2] = {0xd201000000010000ull, 0};
    static constexpr int HARD_N = 20;                   // (q^4 - q^2 + 1) / r
    static constexpr uint64_t HARD[20] = {0xe516c3f438e3ba79ull, 0xfa9912aae208ccf1ull, 0x905ce937335d5b68ull, 0xc71a2629b0dea236ull, 0x83774940996754c8ull,
                                          0x21d160aeb6a1e799ull, 0x2ed0b283ed237db4ull, 0x915c97f36c6f1821ull, 0x67f17fcbde783765ull, 0x2378b9039096d1b7ull,
                                          0x7988f8761bdc51dcull, 0x2076995003fc77a1ull, 0x827eca0ba621315bull, 0xe5a72bce8d63cb9full, 0xf68f7764c28b6f8aull,
                                          0x2f230063cf081517ull, 0x94506632528d6a9aull, 0xd3cde88eeb996ca3ull, 0xc0bd38c3195c899eull, 0x000f686b3d807d01ull};
    static constexpr uint64_t R[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
    // the standard G2 generator: x.c0, x.c1, y.c0, y.c1 (canonical)
    static constexpr uint64_t G2[4][6] = {
        {0xd48056c8c121bdb8ull, 0x0bac0326a805bbefull, 0xb4510b647ae3d177ull, 0xc6e47ad4fa403b02ull, 0x260805272dc51051ull, 0x024aa2b2f08f0a91ull},
        {0xe5ac7d055d042b7eull, 0x334cf11213945d57ull, 0xb5da61bbdc7f5049ull, 0x596bd0d09920b61aull, 0x7dacd3a088274f65ull, 0x13e02b6052719f60ull},
        {0xe193548608b82801ull, 0x923ac9cc3baca289ull, 0x6d429a695160d12cull, 0xadfd9baa8cbdd3a7ull, 0x8cc9cdc6da2e351aull, 0x0ce5d527727d6e11ull},
        {0xaaa9075ff05f79beull, 0x3f370d275cec1da1ull, 0x267492ab572e99abull, 0xcb3e287e85a763afull, 0x32acd2b02bc28b99ull, 0x0606c4a02ea734ccull}};
};
struct Bn254 {
    using P = BnFq;
    static constexpr int N = 4;
    static constexpr int FB = 32;
    static constexpr bool BE = false;                   // records: little-endian, c0 first, flags in the last byte
    static constexpr int XI0 = 9;
    static constexpr bool TWIST_MUL = false;            // b' = b / xi
    static constexpr bool BN_LINES = true, NEG_X = false;
    static constexpr int ATE_BITS = 65;
    static constexpr uint64_t ATE[2] = {0x9d797039be763ba8ull, 1};
    static constexpr int HARD_N = 12;
    static constexpr uint64_t HARD[12] = {0xe81bb482ccdf42b1ull, 0x5abf5cc4f49c36d4ull, 0xf1154e7e1da014fdull, 0xdcc7b44c87cdbacfull, 0xaaa441e3954bcf8aull,
                                          0x6b887d56d5095f23ull, 0x79581e16f3fd90c6ull, 0x3b1b1355d189227dull, 0x4e529a5861876f6bull, 0x6c0eb522d5b12278ull,
                                          0x331ec15183177fafull, 0x01baaa710b0759adull};
    static constexpr uint64_t R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    static constexpr uint64_t G2[4][4] = {{0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull},
                                          {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull},
                                          {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull},
                                          {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull}};
};

// ---- Fq helpers -----------------------------------------------------------------------------------------------------------------------
template <class C> using Fq = Fp64<typename C::P>;

template <class C>
Fq<C> fq_from_canonical(const uint64_t* limbs) {
    Fq<C> a, r2;
    for (int i = 0; i < C::N; i++) { a.l[i] = limbs[i]; r2.l[i] = Fq<C>::c64(C::P::R2, i); }
    return a * r2;
}
template <class C>
Fq<C> fq_small(int k) { return h64::from_u64<typename C::P>((uint64_t)k); }
template <class C>
Fq<C> fq_pow(Fq<C> b, const uint64_t* e, int n) {
    Fq<C> acc = Fq<C>::one();
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 64; k++) {
            if ((e[i] >> k) & 1) acc = acc * b;
            b = b * b;
        }
    return acc;
}
// (q + add) / d for small add, d (exact or floored), into out[C::N]
template <class C>
void q_plus_div(int add, unsigned d, uint64_t* out) {
    uint64_t t[C::N];
    for (int i = 0; i < C::N; i++) t[i] = Fq<C>::mod(i);
    if (add >= 0) { unsigned __int128 c = (unsigned)add; for (int i = 0; i < C::N; i++) { c += t[i]; t[i] = (uint64_t)c; c >>= 64; } }
    else { uint64_t b = (uint64_t)(-add); for (int i = 0; i < C::N; i++) { const uint64_t v = t[i]; t[i] = v - b; b = v < b; } }
    unsigned __int128 rem = 0;
    for (int i = C::N - 1; i >= 0; i--) {
        const unsigned __int128 cur = (rem << 64) | t[i];
        out[i] = (uint64_t)(cur / d);
        rem = cur % d;
    }
}
// a^((q+1)/4): the square root of a square (q = 3 mod 4 on both curves); the caller checks the candidate
template <class C>
Fq<C> fq_sqrt_candidate(const Fq<C>& a) {
    uint64_t e[C::N];
    q_plus_div<C>(1, 4, e);
    return fq_pow<C>(a, e, C::N);
}
// -1, 0, 1 on canonical integers
template <class C>
int fq_cmp(const Fq<C>& a, const Fq<C>& b) {
    const auto x = h64::canonical(a), y = h64::canonical(b);
    for (int i = C::N - 1; i >= 0; i--)
        if (x[i] != y[i]) return x[i] > y[i] ? 1 : -1;
    return 0;
}

// ---- Fq2 ------------------------------------------------------------------------------------------------------------------------------
template <class C>
struct Fq2 {
    Fq<C> c0, c1;
    static Fq2 zero() { return {Fq<C>::zero(), Fq<C>::zero()}; }
    static Fq2 one() { return {Fq<C>::one(), Fq<C>::zero()}; }
    bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    bool operator==(const Fq2& o) const { return c0 == o.c0 && c1 == o.c1; }
    friend Fq2 operator+(const Fq2& a, const Fq2& b) { return {a.c0 + b.c0, a.c1 + b.c1}; }
    friend Fq2 operator-(const Fq2& a, const Fq2& b) { return {a.c0 - b.c0, a.c1 - b.c1}; }
    friend Fq2 operator*(const Fq2& a, const Fq2& b) {
        const Fq<C> t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
        return {t0 - t1, (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1};
    }
};
template <class C> Fq2<C> neg(const Fq2<C>& a) { return {neg(a.c0), neg(a.c1)}; }
template <class C> Fq2<C> conj(const Fq2<C>& a) { return {a.c0, neg(a.c1)}; }
template <class C> Fq2<C> sqr(const Fq2<C>& a) { const Fq<C> t = a.c0 * a.c1; return {(a.c0 + a.c1) * (a.c0 - a.c1), t + t}; }
template <class C> Fq2<C> scale(const Fq2<C>& a, const Fq<C>& k) { return {a.c0 * k, a.c1 * k}; }
template <class C> Fq2<C> dbl(const Fq2<C>& a) { return a + a; }
template <class C> Fq<C> mul_small(const Fq<C>& a, int k) {          // k a for a small constant, by doubling
    Fq<C> acc = Fq<C>::zero(), b = a;
    for (; k; k >>= 1) { if (k & 1) acc = acc + b; b = b + b; }
    return acc;
}
template <class C> Fq2<C> mul_xi(const Fq2<C>& a) { return {mul_small<C>(a.c0, C::XI0) - a.c1, mul_small<C>(a.c1, C::XI0) + a.c0}; }
template <class C> Fq2<C> inv(const Fq2<C>& a) {                      // inv(0) = 0
    const Fq<C> n = h64::inv(a.c0 * a.c0 + a.c1 * a.c1);
    return {a.c0 * n, neg(a.c1 * n)};
}
template <class C> Fq2<C> fq2_pow(Fq2<C> b, const uint64_t* e, int n) {
    Fq2<C> acc = Fq2<C>::one();
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 64; k++) {
            if ((e[i] >> k) & 1) acc = acc * b;
            b = sqr(b);
        }
    return acc;
}
template <class C> Fq2<C> xi() { return {fq_small<C>(C::XI0), Fq<C>::one()}; }
// the twist's constant term: b xi or b / xi
template <class C> Fq2<C> twist_b() {
    const Fq2<C> b{Fq<C>::from_words(C::P::CURVE_B), Fq<C>::zero()};
    return C::TWIST_MUL ? b * xi<C>() : b * inv(xi<C>());
}
// a square root of a, false when a is no square: by the norm (sqrt of a0 + a1 u is x0 + x1 u with x0^2 = (a0 +- sqrt(a0^2 + a1^2)) / 2, x1 = a1 / 2 x0)
template <class C> bool fq2_sqrt(const Fq2<C>& a, Fq2<C>& out) {
    if (a.is_zero()) { out = a; return true; }
    Fq2<C> cand;
    if (a.c1.is_zero()) {
        const Fq<C> s = fq_sqrt_candidate<C>(a.c0);
        if (s * s == a.c0) cand = {s, Fq<C>::zero()};
        else cand = {Fq<C>::zero(), fq_sqrt_candidate<C>(neg(a.c0))};               // a0 a non-residue: -a0 is a square, (s u)^2 = -s^2
    } else {
        const Fq<C> n = a.c0 * a.c0 + a.c1 * a.c1, s = fq_sqrt_candidate<C>(n);
        if (!(s * s == n)) return false;
        const Fq<C> half = h64::inv(fq_small<C>(2));
        Fq<C> t = (a.c0 + s) * half, x0 = fq_sqrt_candidate<C>(t);
        if (!(x0 * x0 == t)) { t = (a.c0 - s) * half; x0 = fq_sqrt_candidate<C>(t); }
        cand = {x0, a.c1 * h64::inv(x0 + x0)};
    }
    if (!(sqr(cand) == a)) return false;
    out = cand;
    return true;
}
// "y is the larger" of ark's SWFlags on Fq2: y > -y, c1 compared first, then c0
template <class C> bool fq2_is_larger(const Fq2<C>& y) {
    const Fq2<C> m = neg(y);
    const int k = fq_cmp<C>(y.c1, m.c1);
    return k ? k > 0 : fq_cmp<C>(y.c0, m.c0) > 0;
}

// ---- Fq6, Fq12 ------------------------------------------------------------------------------------------------------------------------
template <class C>
struct Fq6 {
    Fq2<C> c0, c1, c2;
    static Fq6 zero() { return {Fq2<C>::zero(), Fq2<C>::zero(), Fq2<C>::zero()}; }
    static Fq6 one() { return {Fq2<C>::one(), Fq2<C>::zero(), Fq2<C>::zero()}; }
    bool operator==(const Fq6& o) const { return c0 == o.c0 && c1 == o.c1 && c2 == o.c2; }
    friend Fq6 operator+(const Fq6& a, const Fq6& b) { return {a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2}; }
    friend Fq6 operator-(const Fq6& a, const Fq6& b) { return {a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2}; }
    friend Fq6 operator*(const Fq6& a, const Fq6& b) {
        const Fq2<C> t0 = a.c0 * b.c0, t1 = a.c1 * b.c1, t2 = a.c2 * b.c2;
        return {t0 + mul_xi((a.c1 + a.c2) * (b.c1 + b.c2) - t1 - t2), (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1 + mul_xi(t2),
                (a.c0 + a.c2) * (b.c0 + b.c2) - t0 - t2 + t1};
    }
};
template <class C> Fq6<C> neg(const Fq6<C>& a) { return {neg(a.c0), neg(a.c1), neg(a.c2)}; }
template <class C> Fq6<C> mul_v(const Fq6<C>& a) { return {mul_xi(a.c2), a.c0, a.c1}; }
template <class C> Fq6<C> inv(const Fq6<C>& a) {
    const Fq2<C> A = sqr(a.c0) - mul_xi(a.c1 * a.c2), B = mul_xi(sqr(a.c2)) - a.c0 * a.c1, D = sqr(a.c1) - a.c0 * a.c2;
    const Fq2<C> f = inv(a.c0 * A + mul_xi(a.c2 * B + a.c1 * D));
    return {A * f, B * f, D * f};
}

template <class C>
struct Fq12 {
    Fq6<C> c0, c1;
    static Fq12 one() { return {Fq6<C>::one(), Fq6<C>::zero()}; }
    bool operator==(const Fq12& o) const { return c0 == o.c0 && c1 == o.c1; }
    friend Fq12 operator*(const Fq12& a, const Fq12& b) {
        const Fq6<C> t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
        return {t0 + mul_v(t1), (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1};
    }
    // the coefficient of w^k, k = 0..5, in Fq2: the element is sum g_k w^k
    Fq2<C>& g(int k) { Fq6<C>& h = (k & 1) ? c1 : c0; return (k >> 1) == 0 ? h.c0 : (k >> 1) == 1 ? h.c1 : h.c2; }
    const Fq2<C>& g(int k) const { return const_cast<Fq12*>(this)->g(k); }
};
template <class C> Fq12<C> sqr(const Fq12<C>& a) {
    const Fq6<C> ab = a.c0 * a.c1;
    return {(a.c0 + a.c1) * (a.c0 + mul_v(a.c1)) - ab - mul_v(ab), ab + ab};
}
template <class C> Fq12<C> conj(const Fq12<C>& a) { return {a.c0, neg(a.c1)}; }                 // a^(q^6)
template <class C> Fq12<C> inv(const Fq12<C>& a) {
    const Fq6<C> t = inv(a.c0 * a.c0 - mul_v(a.c1 * a.c1));
    return {a.c0 * t, neg(a.c1 * t)};
}
// xi^((q - 1) / d) for d = 2, 3, 6 (q = 1 mod 6 on both curves)
template <class C> Fq2<C> xi_pow_q1_over(unsigned d) {
    uint64_t e[C::N];
    q_plus_div<C>(-1, d, e);
    return fq2_pow<C>(xi<C>(), e, C::N);
}
// a^(q^2): w^(q^2) = gamma w with gamma = xi^((q^2 - 1) / 6) = Norm(xi^((q - 1) / 6)) in Fq
template <class C> Fq12<C> frobenius2(const Fq12<C>& a) {
    static const Fq<C> gamma = [] { const Fq2<C> t = xi_pow_q1_over<C>(6); return t.c0 * t.c0 + t.c1 * t.c1; }();
    Fq12<C> r = a;
    Fq<C> gk = gamma;
    for (int k = 1; k < 6; k++) { r.g(k) = scale(a.g(k), gk); gk = gk * gamma; }
    return r;
}
template <class C> Fq12<C> fq12_pow(const Fq12<C>& b, const uint64_t* e, int n) {   // 4-bit windows, most significant first
    Fq12<C> tab[16];
    tab[0] = Fq12<C>::one();
    for (int i = 1; i < 16; i++) tab[i] = tab[i - 1] * b;
    Fq12<C> acc = Fq12<C>::one();
    for (int i = n - 1; i >= 0; i--)
        for (int s = 60; s >= 0; s -= 4) {
            acc = sqr(sqr(sqr(sqr(acc))));
            const unsigned d = (unsigned)(e[i] >> s) & 15u;
            if (d) acc = acc * tab[d];
        }
    return acc;
}
template <class C> Fq12<C> final_exponentiation(const Fq12<C>& f) {                    // f^((q^12 - 1) / r); f != 0
    Fq12<C> t = conj(f) * inv(f);
    t = frobenius2(t) * t;
    return fq12_pow<C>(t, C::HARD, C::HARD_N);
}
// the 12 coefficients in the basis 1, w, .., w^11 of Fq[w] / (w^12 - 2 xi0 w^6 + xi0^2 + 1), where u = w^6 - xi0
template <class C> void fq12_power_basis(const Fq12<C>& a, Fq<C>* out) {
    for (int k = 0; k < 6; k++) {
        out[k] = a.g(k).c0 - mul_small<C>(a.g(k).c1, C::XI0);
        out[k + 6] = a.g(k).c1;
    }
}

// ---- G2: affine points of the twist ---------------------------------------------------------------------------------------------------
template <class C>
struct G2 {
    Fq2<C> x, y;
    bool inf;
    static G2 infinity() { return {Fq2<C>::zero(), Fq2<C>::zero(), true}; }
};
template <class C> G2<C> g2_generator() {
    return {{fq_from_canonical<C>(C::G2[0]), fq_from_canonical<C>(C::G2[1])}, {fq_from_canonical<C>(C::G2[2]), fq_from_canonical<C>(C::G2[3])}, false};
}
template <class C> bool g2_on_curve(const G2<C>& p) { return p.inf || sqr(p.y) == sqr(p.x) * p.x + twist_b<C>(); }
template <class C> G2<C> g2_neg(const G2<C>& p) { return {p.x, neg(p.y), p.inf}; }
// the chord / tangent step: R = a + b and the slope used (set only when the line is not vertical)
template <class C> G2<C> g2_add(const G2<C>& a, const G2<C>& b, Fq2<C>* slope = nullptr) {
    if (a.inf) return b;
    if (b.inf) return a;
    Fq2<C> l;
    if (a.x == b.x) {
        if (!(a.y == b.y) || a.y.is_zero()) return G2<C>::infinity();
        const Fq2<C> x2 = sqr(a.x);
        l = (x2 + x2 + x2) * inv(a.y + a.y);
    } else {
        l = (b.y - a.y) * inv(b.x - a.x);
    }
    if (slope) *slope = l;
    const Fq2<C> x3 = sqr(l) - a.x - b.x;
    return {x3, l * (a.x - x3) - a.y, false};
}
template <class C> G2<C> g2_mul(const G2<C>& p, const uint64_t* k, int n) {
    G2<C> acc = G2<C>::infinity();
    for (int i = n - 1; i >= 0; i--)
        for (int b = 63; b >= 0; b--) {
            acc = g2_add(acc, acc);
            if ((k[i] >> b) & 1) acc = g2_add(acc, p);
        }
    return acc;
}
template <class C> bool g2_in_subgroup(const G2<C>& p) { return g2_mul(p, C::R, 4).inf; }

// ---- the pairing ----------------------------------------------------------------------------------------------------------------------
// the line through t with twist slope l at P = (xp, yp), see the header
template <class C> Fq12<C> line_at(const G2<C>& t, const Fq2<C>& l, const Fq<C>& xp, const Fq<C>& yp) {
    Fq12<C> r{Fq6<C>::zero(), Fq6<C>::zero()};
    const Fq2<C> c = l * t.x - t.y, lx = neg(scale(l, xp)), y{yp, Fq<C>::zero()};
    if (C::TWIST_MUL) { r.g(0) = c; r.g(2) = lx; r.g(3) = y; }
    else { r.g(0) = y; r.g(1) = lx; r.g(3) = c; }
    return r;
}
// t <- t + q (t = q: doubling) and the line of that step at P.  The verticals (t = -q, or a point of order 2) cannot occur for q in G2
// during the loops below; should they, the step contributes 1 and t becomes infinity.
template <class C> Fq12<C> line_step(G2<C>& t, const G2<C>& q, const Fq<C>& xp, const Fq<C>& yp) {
    Fq2<C> l;
    const G2<C> was = t;
    t = g2_add(was, q, &l);
    if (was.inf || q.inf || t.inf) return Fq12<C>::one();
    return line_at(was, l, xp, yp);
}
// pi(Q) in twist coordinates (BN254): (conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2))
template <class C> G2<C> g2_frobenius(const G2<C>& q) {
    static const Fq2<C> gx = xi_pow_q1_over<C>(3), gy = xi_pow_q1_over<C>(2);
    return {conj(q.x) * gx, conj(q.y) * gy, q.inf};
}
// the Miller value f_{ate, Q}(P); P = (xp, yp) affine and not infinity, Q in G2
template <class C> Fq12<C> miller_loop(const G2<C>& q, const Fq<C>& xp, const Fq<C>& yp) {
    if (q.inf) return Fq12<C>::one();
    G2<C> t = q;
    Fq12<C> f = Fq12<C>::one();
    for (int i = C::ATE_BITS - 2; i >= 0; i--) {
        f = sqr(f) * line_step(t, t, xp, yp);
        if ((C::ATE[i >> 6] >> (i & 63)) & 1) f = f * line_step(t, q, xp, yp);
    }
    if (C::BN_LINES) {
        const G2<C> q1 = g2_frobenius(q), nq2 = g2_neg(g2_frobenius(q1));
        f = f * line_step(t, q1, xp, yp);
        f = f * line_step(t, nq2, xp, yp);
    }
    return C::NEG_X ? conj(f) : f;
}
// prod e(P_i, Q_i) over n pairs: G1 points as (x, y) Montgomery, (0, 0) = infinity (contributes 1)
template <class C> Fq12<C> multi_pairing(const Fq<C>* g1_xy, const G2<C>* g2, uint64_t n) {
    Fq12<C> f = Fq12<C>::one();
    for (uint64_t i = 0; i < n; i++) {
        if (g1_xy[2 * i].is_zero() && g1_xy[2 * i + 1].is_zero()) continue;
        f = f * miller_loop(g2[i], g1_xy[2 * i], g1_xy[2 * i + 1]);
    }
    return final_exponentiation(f);
}

// ---- G2 records (ark-serialize 0.4) ---------------------------------------------------------------------------------------------------
//   BLS12-381  compressed    96 B  x.c1 || x.c0 big-endian; byte 0: 0x80 compressed (must be set), 0x40 infinity, 0x20 y is the larger
//              uncompressed 192 B  x.c1 || x.c0 || y.c1 || y.c0; byte 0: 0x80 and 0x20 must be clear, 0x40 infinity
//   BN254      compressed    64 B  x.c0 || x.c1 little-endian; last byte: 0x80 y is the larger, 0x40 infinity, both = invalid
//              uncompressed 128 B  x.c0 || x.c1 || y.c0 || y.c1; the flags in the last byte (0x80 ignored on read)
// The checks and their order are those of the G1 decoder (srs_io.cuh; the codes are SrsBad's): flags, infinity (always refused), range,
// square (compressed) or -- with `validate` -- on-curve (uncompressed), then with `validate` [r]Q = O.
enum G2Bad : int { G2_BAD_FLAGS = 0, G2_BAD_RANGE, G2_BAD_SQUARE, G2_BAD_CURVE, G2_BAD_SUBGROUP, G2_BAD_INFINITY };

template <class C> uint64_t g2_record_bytes(bool compressed) { return (uint64_t)C::FB * (compressed ? 2 : 4); }
template <class C> void fq_read(const uint8_t* p, uint64_t* limbs) {                // an Fq image -> its integer, flag bits included
    for (int i = 0; i < C::N; i++) limbs[i] = 0;
    for (int s = 0; s < C::FB; s++) limbs[s >> 3] |= (uint64_t)p[C::BE ? C::FB - 1 - s : s] << (8 * (s & 7));
}
template <class C> void fq_write(const Fq<C>& a, uint8_t* p) {
    const auto v = h64::canonical(a);
    for (int s = 0; s < C::FB; s++) p[C::BE ? C::FB - 1 - s : s] = (uint8_t)(v[s >> 3] >> (8 * (s & 7)));
}
template <class C> bool limbs_below_q(const uint64_t* t) { return !Fq<C>::geq_mod(t); }

// -1, or the first G2Bad that applies
template <class C> int g2_decode(const uint8_t* rec, bool compressed, bool validate, G2<C>& out) {
    constexpr int B = C::FB;
    const int n_fq = compressed ? 2 : 4;
    uint64_t w[4][C::N];
    for (int i = 0; i < n_fq; i++) fq_read<C>(rec + i * B, w[i]);
    bool inf, larger;
    if (C::BE) {
        const unsigned f = rec[0];
        if (compressed ? !(f & 0x80u) : (f & 0xA0u) != 0) return G2_BAD_FLAGS;
        inf = f & 0x40u;
        larger = f & 0x20u;
        w[0][C::N - 1] &= 0x1FFFFFFFFFFFFFFFull;
    } else {
        const unsigned f = rec[n_fq * B - 1];
        if ((f & 0xC0u) == 0xC0u) return G2_BAD_FLAGS;
        inf = f & 0x40u;
        larger = f & 0x80u;
        w[n_fq - 1][C::N - 1] &= 0x3FFFFFFFFFFFFFFFull;
    }
    if (inf) return G2_BAD_INFINITY;
    for (int i = 0; i < n_fq; i++)
        if (!limbs_below_q<C>(w[i])) return G2_BAD_RANGE;
    // record order -> (c0, c1)
    const int i0 = C::BE ? 1 : 0, i1 = C::BE ? 0 : 1;
    G2<C> p;
    p.inf = false;
    p.x = {fq_from_canonical<C>(w[i0]), fq_from_canonical<C>(w[i1])};
    const Fq2<C> rhs = sqr(p.x) * p.x + twist_b<C>();
    if (compressed) {
        Fq2<C> y;
        if (!fq2_sqrt<C>(rhs, y)) return G2_BAD_SQUARE;
        p.y = fq2_is_larger<C>(y) == larger ? y : neg(y);
    } else {
        p.y = {fq_from_canonical<C>(w[2 + i0]), fq_from_canonical<C>(w[2 + i1])};
        if (validate && !(sqr(p.y) == rhs)) return G2_BAD_CURVE;
    }
    if (validate && !g2_in_subgroup(p)) return G2_BAD_SUBGROUP;
    out = p;
    return -1;
}
template <class C> void g2_encode(const G2<C>& p, bool compressed, uint8_t* rec) {
    constexpr int B = C::FB;
    const int n_fq = compressed ? 2 : 4;
    std::memset(rec, 0, (size_t)n_fq * B);
    const bool larger = !p.inf && fq2_is_larger<C>(p.y);
    if (!p.inf) {
        const int i0 = C::BE ? 1 : 0, i1 = C::BE ? 0 : 1;
        fq_write<C>(p.x.c0, rec + i0 * B);
        fq_write<C>(p.x.c1, rec + i1 * B);
        if (!compressed) { fq_write<C>(p.y.c0, rec + (2 + i0) * B); fq_write<C>(p.y.c1, rec + (2 + i1) * B); }
    }
    if (C::BE) rec[0] |= (uint8_t)((compressed ? 0x80u : 0u) | (p.inf ? 0x40u : 0u) | (compressed && larger ? 0x20u : 0u));
    else rec[n_fq * B - 1] |= (uint8_t)((p.inf ? 0x40u : 0u) | (larger ? 0x80u : 0u));
}

}  // namespace hpair
}  // namespace mzk
