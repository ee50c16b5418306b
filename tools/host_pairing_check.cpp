// host_pairing_check.cpp -- csrc/hostpairing.hpp and csrc/merlin.cuh as a stand-alone host program, both curves, seeded inputs:
//   towers      a * inv(a) = 1 in Fq2, Fq6, Fq12; sqr(a) = a * a; (a b) c = a (b c); a (b + c) = a b + a c; frobenius2(a) = a^(q^2) by the power
//   G2          the generator is on the twist and has order r; [a]Q + [b]Q = [a + b]Q; records decode(encode(Q)) = Q in both modes
//   pairing     e = e(G1, G2) != 1, e^r = 1, e([a]P, [b]Q) = e^(a b), e(P, Q1 + Q2) = e(P, Q1) e(P, Q2), e(P, Q) e(-P, Q) = 1 as one product
//   transcript  merlin's own known answer ("test protocol" / "some label" / "challenge")
// then, with `time`, the cost of one Miller loop, one final exponentiation and the verifier's two-pairing product.  No GPU.
// tests/test_pairing_host.py builds it with -fsanitize=undefined,address and runs it.
//   g++ -O2 -std=c++17 -I../mpc-jellyfish_amd/csrc -o host_pairing_check host_pairing_check.cpp && ./host_pairing_check [n_random] [time]
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "hostpairing.hpp"
#include "merlin.cuh"

using namespace mzk;
using namespace mzk::hpair;

static uint64_t rng_state = 0x6d7a6b5f70616972ull;
static uint64_t next64() {                                   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static int failures = 0;
#define CHECK(cond, what)                                                   \
    do {                                                                    \
        if (!(cond)) { failures++; std::printf("FAIL %s: %s\n", name, what); } \
    } while (0)

template <class C> static Fq<C> rand_fq() {
    uint64_t t[C::N];
    do {
        for (int i = 0; i < C::N; i++) t[i] = next64();
        t[C::N - 1] &= ~0ull >> (64 * C::N - C::P::BITS);
    } while (Fq<C>::geq_mod(t));
    return fq_from_canonical<C>(t);
}
template <class C> static Fq2<C> rand_fq2() { return {rand_fq<C>(), rand_fq<C>()}; }
template <class C> static Fq6<C> rand_fq6() { return {rand_fq2<C>(), rand_fq2<C>(), rand_fq2<C>()}; }
template <class C> static Fq12<C> rand_fq12() { return {rand_fq6<C>(), rand_fq6<C>()}; }

// G1, affine, for the test's own [a]P (x = y = 0: infinity)
template <class C> struct G1 { Fq<C> x, y; bool inf; };
template <class C> static G1<C> g1_add(const G1<C>& a, const G1<C>& b) {
    if (a.inf) return b;
    if (b.inf) return a;
    Fq<C> l;
    if (a.x == b.x) {
        if (!(a.y == b.y)) return {Fq<C>::zero(), Fq<C>::zero(), true};
        const Fq<C> x2 = a.x * a.x;
        l = (x2 + x2 + x2) * h64::inv(a.y + a.y);
    } else {
        l = (b.y - a.y) * h64::inv(b.x - a.x);
    }
    const Fq<C> x3 = l * l - a.x - b.x;
    return {x3, l * (a.x - x3) - a.y, false};
}
template <class C> static G1<C> g1_mul(const G1<C>& p, uint64_t k) {
    G1<C> acc{Fq<C>::zero(), Fq<C>::zero(), true};
    for (int b = 63; b >= 0; b--) {
        acc = g1_add(acc, acc);
        if ((k >> b) & 1) acc = g1_add(acc, p);
    }
    return acc;
}
template <class C> static Fq12<C> pairing(const G1<C>& p, const G2<C>& q) {
    const Fq<C> xy[2] = {p.x, p.y};
    return multi_pairing<C>(xy, &q, 1);
}

template <class C> static void check(const char* name, int n_random, bool timing) {
    // ---- towers
    uint64_t q2e[2 * C::N] = {};                                  // q^2, for the Frobenius check
    for (int i = 0; i < C::N; i++) {
        unsigned __int128 c = 0;
        for (int j = 0; j < C::N; j++) {
            c += (unsigned __int128)Fq<C>::mod(i) * Fq<C>::mod(j) + q2e[i + j];
            q2e[i + j] = (uint64_t)c;
            c >>= 64;
        }
        q2e[i + C::N] = (uint64_t)c;
    }
    for (int it = 0; it < n_random; it++) {
        const Fq2<C> a2 = rand_fq2<C>(), b2 = rand_fq2<C>();
        CHECK(a2 * inv(a2) == Fq2<C>::one(), "Fq2 inverse");
        CHECK(sqr(a2) == a2 * a2 && a2 * b2 == b2 * a2, "Fq2 square / commutativity");
        Fq2<C> root;
        CHECK(fq2_sqrt<C>(sqr(a2), root) && (root == a2 || root == neg(a2)), "Fq2 square root");
        const Fq6<C> a6 = rand_fq6<C>(), b6 = rand_fq6<C>(), c6 = rand_fq6<C>();
        CHECK(a6 * inv(a6) == Fq6<C>::one(), "Fq6 inverse");
        CHECK((a6 * b6) * c6 == a6 * (b6 * c6) && a6 * (b6 + c6) == a6 * b6 + a6 * c6, "Fq6 ring laws");
        Fq6<C> v6 = Fq6<C>::zero();
        v6.c1 = Fq2<C>::one();
        CHECK(mul_v(a6) == a6 * v6, "Fq6 times v");
        const Fq12<C> a = rand_fq12<C>(), b = rand_fq12<C>(), c = rand_fq12<C>();
        CHECK(a * inv(a) == Fq12<C>::one(), "Fq12 inverse");
        CHECK(sqr(a) == a * a && (a * b) * c == a * (b * c), "Fq12 square / associativity");
        if (it < 2) {
            Fq12<C> p = Fq12<C>::one(), base = a;                 // a^(q^2), bit by bit
            for (int i = 0; i < 2 * C::N; i++)
                for (int k = 0; k < 64; k++) { if ((q2e[i] >> k) & 1) p = p * base; base = sqr(base); }
            CHECK(frobenius2(a) == p, "Fq12 Frobenius^2");
            Fq12<C> c6p = a;                                      // a^(q^6) = conj(a): three Frobenius^2
            for (int i = 0; i < 3; i++) c6p = frobenius2(c6p);
            CHECK(c6p == conj(a), "Fq12 conjugate");
        }
    }
    // ---- G2
    const G2<C> g2 = g2_generator<C>();
    CHECK(g2_on_curve(g2), "G2 generator on the twist");
    CHECK(g2_in_subgroup(g2), "G2 generator of order r");
    const uint64_t ka[4] = {next64(), next64(), 0, 0}, kb[4] = {next64(), next64(), 0, 0};
    uint64_t kab[4] = {};
    { unsigned __int128 s = 0; for (int i = 0; i < 3; i++) { s += (unsigned __int128)ka[i] + kb[i]; kab[i] = (uint64_t)s; s >>= 64; } }
    const G2<C> qa = g2_mul(g2, ka, 4), qb = g2_mul(g2, kb, 4), qab = g2_add(qa, qb), want = g2_mul(g2, kab, 4);
    CHECK(g2_on_curve(qa) && qab.x == want.x && qab.y == want.y && !qab.inf, "G2 [a]Q + [b]Q = [a + b]Q");
    for (int compressed = 0; compressed < 2; compressed++) {
        uint8_t rec[4 * C::FB];
        G2<C> back;
        g2_encode<C>(qa, compressed, rec);
        CHECK(g2_decode<C>(rec, compressed, true, back) == -1 && back.x == qa.x && back.y == qa.y, "G2 record round trip");
        g2_encode<C>(g2_neg(qa), compressed, rec);
        CHECK(g2_decode<C>(rec, compressed, true, back) == -1 && back.x == qa.x && back.y == neg(qa.y), "G2 record round trip (-Q)");
    }
    // ---- pairing
    const G1<C> g1{Fq<C>::from_words(C::P::GEN_X), Fq<C>::from_words(C::P::GEN_Y), false};
    const Fq12<C> e = pairing<C>(g1, g2), one = Fq12<C>::one();
    CHECK(!(e == one), "e(G1, G2) != 1");
    {
        Fq12<C> p = one, base = e;
        for (int i = 0; i < 4; i++)
            for (int k = 0; k < 64; k++) { if ((C::R[i] >> k) & 1) p = p * base; base = sqr(base); }
        CHECK(p == one, "e(G1, G2)^r = 1");
    }
    const uint64_t a = 0x1234567, b[4] = {0x89abcde, 0, 0, 0}, ab[1] = {a * 0x89abcdeull};
    const G1<C> pa = g1_mul(g1, a);
    const G2<C> qbb = g2_mul(g2, b, 4);
    CHECK(pairing<C>(pa, qbb) == fq12_pow<C>(e, ab, 1), "e([a]P, [b]Q) = e(P, Q)^(a b)");
    CHECK(pairing<C>(pa, qab) == pairing<C>(pa, qa) * pairing<C>(pa, qb), "e(P, Q1 + Q2) = e(P, Q1) e(P, Q2)");
    {
        const Fq<C> xy[6] = {pa.x, pa.y, pa.x, neg(pa.y), Fq<C>::zero(), Fq<C>::zero()};
        const G2<C> qs[3] = {qa, qa, qb};
        CHECK(multi_pairing<C>(xy, qs, 3) == one, "e(P, Q) e(-P, Q) e(O, Q') = 1");
        CHECK(!(multi_pairing<C>(xy, qs, 1) == one) && multi_pairing<C>(xy, qs, 0) == one, "one pair != 1, no pair = 1");
    }
    if (timing) {
        using clk = std::chrono::steady_clock;
        const int reps = 20;
        const Fq<C> xy[4] = {pa.x, pa.y, g1.x, neg(g1.y)};
        const G2<C> qs[2] = {qa, qb};
        Fq12<C> f = one;
        auto t0 = clk::now();
        for (int i = 0; i < reps; i++) f = f * miller_loop<C>(qa, pa.x, pa.y);
        auto t1 = clk::now();
        for (int i = 0; i < reps; i++) f = final_exponentiation<C>(f * e);
        auto t2 = clk::now();
        int acc = 0;
        for (int i = 0; i < reps; i++) acc += multi_pairing<C>(xy, qs, 2) == one;
        auto t3 = clk::now();
        const auto ms = [&](clk::time_point x, clk::time_point y) { return std::chrono::duration<double, std::milli>(y - x).count() / reps; };
        std::printf("%s: Miller loop %.3f ms, final exponentiation %.3f ms, two-pairing product %.3f ms (%d%d)\n", name, ms(t0, t1), ms(t1, t2), ms(t2, t3),
                    acc, (int)(f == one));
    }
    std::printf("%s: %d random tower cases checked\n", name, n_random);
}

static void check_merlin() {
    const char* name = "merlin";
    uint64_t lanes[25];
    merlin::Transcript t;
    t.init(lanes, 1, "test protocol", 13);
    t.append_message("some label", 10, (const uint8_t*)"some data", 9);
    uint8_t out[32];
    t.challenge_bytes("challenge", 9, out, 32);
    char hex[65];
    for (int i = 0; i < 32; i++) std::snprintf(hex + 2 * i, 3, "%02x", out[i]);
    CHECK(std::strcmp(hex, "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615") == 0, "known answer");
}

int main(int argc, char** argv) {
    const int n_random = argc > 1 ? std::atoi(argv[1]) : 50;
    const bool timing = argc > 2 && std::strcmp(argv[2], "time") == 0;
    check<Bls12>("BLS12-381", n_random, timing);
    check<Bn254>("BN254", n_random, timing);
    check_merlin();
    std::printf(failures ? "FAILED\n" : "ok\n");
    return failures ? 1 : 0;
}
