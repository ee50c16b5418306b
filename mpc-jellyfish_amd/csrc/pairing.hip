// pairing.hip -- the host-only entry points over hostpairing.hpp and merlin.cuh: G2 records, [k]Q, the pairing product of the verifier's
// final check and its batch challenge r.  No kernel, no HIP call: they run without a GPU and before mzk_init, like mzk_key_layout.
#include "internal.hpp"
#include "hostpairing.hpp"
#include "keccak_transcript.cuh"
#include "merlin.cuh"

namespace mzk {
namespace {

using namespace hpair;

template <class C>
int32_t g2_decode_entry(const uint8_t* bytes, uint32_t flags, G2<C>& out) {
    const int bad = g2_decode<C>(bytes, flags & MZK_SER_COMPRESSED, flags & MZK_SER_VALIDATE, out);
    if (bad < 0) return MZK_OK;
    set_error(std::string("G2: ") + srs_bad_reason(bad));              // (G2Bad numbers its reasons as the G1 decoder's SrsBad)
    return MZK_ERR_ENCODING;
}
template <class C>
void g2_store(const G2<C>& p, uint64_t* out) {
    const Fq<C>* f[4] = {&p.x.c0, &p.x.c1, &p.y.c0, &p.y.c1};
    for (int i = 0; i < 4; i++) std::memcpy(out + i * C::N, f[i]->l, sizeof f[i]->l);
}
template <class C>
G2<C> g2_load(const uint64_t* in) {
    G2<C> p;
    Fq<C>* f[4] = {&p.x.c0, &p.x.c1, &p.y.c0, &p.y.c1};
    for (int i = 0; i < 4; i++) std::memcpy(f[i]->l, in + i * C::N, sizeof f[i]->l);
    p.inf = false;
    return p;
}
template <class C>
int32_t g2_decode_t(const uint8_t* bytes, uint32_t flags, uint64_t* out) {
    G2<C> p;
    MZK_TRY(g2_decode_entry<C>(bytes, flags, p));
    g2_store<C>(p, out);
    return MZK_OK;
}
template <class C>
int32_t g2_mul_t(const uint8_t* q_bytes, const uint64_t* k, uint32_t flags, uint8_t* out) {
    G2<C> q = g2_generator<C>();
    if (q_bytes) MZK_TRY(g2_decode_entry<C>(q_bytes, flags, q));
    g2_encode<C>(g2_mul<C>(q, k, 4), flags & MZK_SER_COMPRESSED, out);
    return MZK_OK;
}
template <class C>
Fq12<C> pairing_product_t(const uint64_t* g1, const uint64_t* g2, uint64_t n) {
    std::vector<Fq<C>> p(2 * n);
    std::vector<G2<C>> q(n);
    for (uint64_t i = 0; i < n; i++) {
        std::memcpy(p[2 * i].l, g1 + 2 * i * C::N, sizeof p[0].l);
        std::memcpy(p[2 * i + 1].l, g1 + (2 * i + 1) * C::N, sizeof p[0].l);
        q[i] = g2_load<C>(g2 + 4 * i * C::N);
    }
    return multi_pairing<C>(p.data(), q.data(), n);
}
template <class C>
void pairing_gt_t(const uint64_t* g1, const uint64_t* g2, uint64_t* out) {
    Fq<C> c[12];
    fq12_power_basis<C>(pairing_product_t<C>(g1, g2, 1), c);
    for (int i = 0; i < 12; i++) {
        const auto v = h64::canonical(c[i]);
        std::memcpy(out + i * C::N, v.data(), sizeof(uint64_t) * C::N);
    }
}

// verifier.rs:203-215; a 64-byte challenge is reduced as lo + 2^256 hi: each half below r by subtraction, then Montgomery products by R^2
template <class FrP>
void batch_challenge_t(const uint64_t* u_mont, uint64_t K, uint64_t* out) {
    using F = Fp64<FrP>;
    if (K == 1) { const F one = F::one(); std::memcpy(out, one.l, sizeof one.l); return; }
    uint64_t lanes[25];
    merlin::Transcript t;
    t.init(lanes, 1, "batch verify", 12);
    for (uint64_t i = 0; i < K; i++) {
        F u;
        std::memcpy(u.l, u_mont + 4 * i, sizeof u.l);
        const auto v = h64::canonical(u);
        uint8_t rec[32];
        for (int s = 0; s < 32; s++) rec[s] = (uint8_t)(v[s >> 3] >> (8 * (s & 7)));
        t.append_message("u", 1, rec, 32);
    }
    uint8_t ch[64];
    t.challenge_bytes("r", 1, ch, 64);
    F lo = F::zero(), hi = F::zero(), r2;
    for (int s = 0; s < 32; s++) { lo.l[s >> 3] |= (uint64_t)ch[s] << (8 * (s & 7)); hi.l[s >> 3] |= (uint64_t)ch[32 + s] << (8 * (s & 7)); }
    for (int i = 0; i < 4; i++) r2.l[i] = F::c64(FrP::R2, i);
    while (F::geq_mod(lo.l)) F::sub_mod(lo.l);                         // (2^256 < 6 r on both curves)
    while (F::geq_mod(hi.l)) F::sub_mod(hi.l);
    const F r = lo * r2 + (hi * r2) * r2;
    std::memcpy(out, r.l, sizeof r.l);
}

// the first 48 bytes of a Solidity transcript's state, little-endian, mod r (solidity.rs:74-76), Montgomery
template <class FrP>
void solidity_reduce_t(const uint8_t* state64, uint64_t* out) {
    using F = Fp64<FrP>;
    F lo = F::zero(), hi = F::zero(), r2;
    for (int s = 0; s < 32; s++) lo.l[s >> 3] |= (uint64_t)state64[s] << (8 * (s & 7));
    for (int s = 0; s < 16; s++) hi.l[s >> 3] |= (uint64_t)state64[32 + s] << (8 * (s & 7));
    for (int i = 0; i < 4; i++) r2.l[i] = F::c64(FrP::R2, i);
    while (F::geq_mod(lo.l)) F::sub_mod(lo.l);
    const F r = lo * r2 + (hi * r2) * r2;                                // (hi < 2^128 < r)
    std::memcpy(out, r.l, sizeof r.l);
}
// verifier.rs:203-215 with T = SolidityTranscript: the K values u as the whole transcript, one challenge
template <class FrP>
void batch_challenge_solidity_t(const uint64_t* u_mont, uint64_t K, uint64_t* out) {
    using F = Fp64<FrP>;
    if (K == 1) { const F one = F::one(); std::memcpy(out, one.l, sizeof one.l); return; }
    std::vector<uint8_t> tr(K * 32);
    for (uint64_t i = 0; i < K; i++) {
        F u;
        std::memcpy(u.l, u_mont + 4 * i, sizeof u.l);
        const auto v = h64::canonical(u);
        for (int s = 0; s < 32; s++) tr[i * 32 + s] = (uint8_t)(v[s >> 3] >> (8 * (s & 7)));
    }
    uint8_t state[64] = {0};
    keccak::solidity_squeeze_bytes(state, tr.data(), tr.size());
    solidity_reduce_t<FrP>(state, out);
}

}  // namespace
}  // namespace mzk

using namespace mzk;

extern "C" int32_t mzk_g2_decode(int32_t curve_id, const uint8_t* bytes, uint32_t flags, uint64_t* out_xy_mont) {
    if (!valid_curve(curve_id) || !bytes || !out_xy_mont) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    return curve_id == MZK_CURVE_BLS12_381 ? g2_decode_t<hpair::Bls12>(bytes, flags, out_xy_mont) : g2_decode_t<hpair::Bn254>(bytes, flags, out_xy_mont);
}

extern "C" int32_t mzk_g2_mul(int32_t curve_id, const uint8_t* q_bytes, const uint64_t* k_canonical, uint32_t flags, uint8_t* out_bytes) {
    if (!valid_curve(curve_id) || !k_canonical || !out_bytes) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    return curve_id == MZK_CURVE_BLS12_381 ? g2_mul_t<hpair::Bls12>(q_bytes, k_canonical, flags, out_bytes)
                                           : g2_mul_t<hpair::Bn254>(q_bytes, k_canonical, flags, out_bytes);
}

extern "C" int32_t mzk_pairing_product_is_one(int32_t curve_id, const uint64_t* g1_xy_mont, const uint64_t* g2_xy_mont, uint64_t n, int32_t* out) {
    if (!valid_curve(curve_id) || !out || (n && (!g1_xy_mont || !g2_xy_mont)) || n > (1ull << 32)) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    if (curve_id == MZK_CURVE_BLS12_381) *out = pairing_product_t<hpair::Bls12>(g1_xy_mont, g2_xy_mont, n) == hpair::Fq12<hpair::Bls12>::one();
    else *out = pairing_product_t<hpair::Bn254>(g1_xy_mont, g2_xy_mont, n) == hpair::Fq12<hpair::Bn254>::one();
    return MZK_OK;
}

extern "C" int32_t mzk_pairing_gt(int32_t curve_id, const uint64_t* g1_xy_mont, const uint64_t* g2_xy_mont, uint64_t* out) {
    if (!valid_curve(curve_id) || !g1_xy_mont || !g2_xy_mont || !out) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    if (curve_id == MZK_CURVE_BLS12_381) pairing_gt_t<hpair::Bls12>(g1_xy_mont, g2_xy_mont, out);
    else pairing_gt_t<hpair::Bn254>(g1_xy_mont, g2_xy_mont, out);
    return MZK_OK;
}

extern "C" int32_t mzk_batch_verify_challenge(int32_t curve_id, const uint64_t* u_mont, uint64_t K, uint64_t* out_r_mont) {
    if (!valid_curve(curve_id) || !u_mont || !K || !out_r_mont) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    if (curve_id == MZK_CURVE_BLS12_381) batch_challenge_t<BlsFr>(u_mont, K, out_r_mont);
    else batch_challenge_t<BnFr>(u_mont, K, out_r_mont);
    return MZK_OK;
}

extern "C" int32_t mzk_batch_verify_challenge_t(int32_t curve_id, uint32_t flags, const uint64_t* u_mont, uint64_t K, uint64_t* out_r_mont) {
    if (flags & ~MZK_TRANSCRIPT_SOLIDITY) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    if (!(flags & MZK_TRANSCRIPT_SOLIDITY)) return mzk_batch_verify_challenge(curve_id, u_mont, K, out_r_mont);
    if (!valid_curve(curve_id) || !u_mont || !K || !out_r_mont) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    if (curve_id == MZK_CURVE_BLS12_381) batch_challenge_solidity_t<BlsFr>(u_mont, K, out_r_mont);
    else batch_challenge_solidity_t<BnFr>(u_mont, K, out_r_mont);
    return MZK_OK;
}

extern "C" int32_t mzk_keccak256(const uint8_t* msg, uint64_t len, uint8_t* out32) {
    if ((!msg && len) || !out32) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    keccak::keccak256(msg, len, out32);
    return MZK_OK;
}

extern "C" int32_t mzk_solidity_challenge(int32_t curve_id, uint8_t* state64, const uint8_t* transcript, uint64_t len, uint64_t* out_mont) {
    if (!valid_curve(curve_id) || !state64 || (!transcript && len) || !out_mont) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    keccak::solidity_squeeze_bytes(state64, transcript, len);
    if (curve_id == MZK_CURVE_BLS12_381) solidity_reduce_t<BlsFr>(state64, out_mont);
    else solidity_reduce_t<BnFr>(state64, out_mont);
    return MZK_OK;
}
