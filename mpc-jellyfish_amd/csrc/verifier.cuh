// verifier.cuh -- the per-proof work of PlonkKzgSnark::batch_verify and verify_batch_proof on the device: K images
// of proof_len bytes, each of m instances under a tuple of m keys of one type, domain and open key.  ONE set of stages serves two image
// layouts, both described by a VfyAggShape and a column table: a `Proof` (structs.rs:59-84; m = 1, the strides unused) and a `BatchProof`
// (structs.rs:266-291; instance j's records at base + j * stride).  Proof links (verify_link_proof) and KZG openings (UnivariateKzgPCS::verify): the last two sections.
//   A  vfy_decode_kernel          one thread per G1 record: the decoder of srs_io.cuh in its infinity-tolerant mode -> the base array;
//                                 offsets and field names from device memory (a key image and a link's four records go through it too)
//   B  vfy_agg_transcript_kernel  one thread per proof: compute_challenges over m keys (verifier.rs:256-321) -> 7 challenges; T is
//                                 merlin::Transcript (StandardTranscript) or keccak::SolidityTranscript (MZK_TRANSCRIPT_SOLIDITY)
//   C  vfy_agg_scalars_kernel     one thread per (proof, instance): that instance's share of prepare_pcs_info (verifier.rs:68-184, 340-733)
//   F  vfy_agg_fold_kernel        one thread per proof: the m shares summed in instance order, the scalars that belong to the whole proof
//   finish                        vfy_weight_kernel / vfy_colsum_kernel: rows weighted by r^i, the key's columns summed by a fixed tree
// Base array (boundary form, what mzk_srs_register_dev takes): [ key bases | proof 0's points | proof 1's points | .. ], in COLUMN order:
//   key columns    position 0's block (selectors (13 | 14), sigmas (W), Ultra: range, key, table_dom_sep, q_dom_sep), position 1's, .., then open_key.g
//   proof columns  j < m: wires_j (W), prod_perm_j | split_quot (W), opening, shifted_opening | Ultra, j < m: h_1, h_2, prod_lookup
// (m = 1: NKEY = nsel + W + 4 ultra + 1, NP = 13 | 18, the image order of a `Proof`).  A base at infinity holds the curve's generator and
// is FLAGGED; the finish zeroes its scalar.
// Errors: one 64-bit atomicMin over (proof << 40 | instance << 33 | field << 4 | reason): the lowest proof, then its lowest instance, then
// its first field, on every run.  A BatchProof counts what belongs to the whole proof as instance m; a `Proof`, a key and a link name
// every record by its index in the image under instance 0.
#pragma once
#include <hip/hip_runtime.h>

#include "fp.cuh"
#include "fp_inv.cuh"
#include "key_io.cuh"                                              // fr_read_record
#include "keccak_transcript.cuh"
#include "merlin.cuh"
#include "srs_io.cuh"

namespace mzk {

#define VFY_LBL(s) s, (uint32_t)(sizeof(s) - 1)                  // a transcript label and its length
constexpr int VFY_THREADS = 64;                                  // one wave; stage B keeps 25 lanes x 64 transcripts = 12.5 KB of LDS
constexpr uint32_t VFY_REASON_NOT_BELOW_R = 6;                   // after SrsBad's six
constexpr uint32_t VFY_FIELD_EVAL = 32, VFY_FIELD_PUB_INPUT = 64;  // fields: 0..24 point j, 32 + e evaluation e, 64 + i public input i
constexpr uint32_t VFY_MAX_INSTANCES = 64;                       // MZK_VERIFIER_MAX_INSTANCES
struct VfyAggShape {                                             // the images of one batch (a `Proof`: m = 1, nkey1 = nkey - 1, no stride read)
    uint32_t m, W, nsel, ultra, np, nkey, nkey1, log_n, compressed, g1_bytes, proof_len, total_inputs;   // nkey1: one position's block
    uint32_t wires_off, wires_stride;                            // instance j's first wire commitment
    uint32_t prod_off;                                           // prod_perm_poly_comms_vec[0]; stride g1_bytes
    uint32_t evals_off, evals_stride;                            // instance j's ProofEvaluations, at the count of wires_evals
    uint32_t plk_off, plk_stride;                                // instance j's Option<PlookupProof>, at its tag
    uint32_t quot_off;                                           // split_quot_poly_comms[0]; opening_proof and shifted_opening_proof follow the W records
    unsigned long long n;
};
// pos_tab, 3 (m + 1) words: per position { byte offset of its script, items of its script, first public input }, then the totals

MZK_D void vfy_agg_report(unsigned long long* err, unsigned long long proof, uint32_t inst, uint32_t field, uint32_t reason) {
    atomicMin(err, (proof << 40) | ((unsigned long long)inst << 33) | ((unsigned long long)field << 4) | reason);
}

// ---- A -------------------------------------------------------------------------------------------------------------------------------
// n_images images `stride` bytes apart, np records each: record j at off[j], reported as fld[j] = instance << 8 | field.  Records open_idx
// and open_idx + 1 also go to a_bases (the MSM A); np names no record, so it stands for "no opening columns" (a_bases is not touched).
template <class X, bool COMPRESSED, bool VALIDATE>
__global__ __launch_bounds__(VFY_THREADS) void vfy_decode_kernel(const uint8_t* __restrict__ images, unsigned long long n_images, uint32_t np, uint32_t stride,
                                                                 const uint32_t* __restrict__ off, const uint32_t* __restrict__ fld, uint32_t open_idx,
                                                                 uint32_t* __restrict__ bases, uint32_t* __restrict__ inf_flags, uint32_t* __restrict__ a_bases,
                                                                 uint32_t* __restrict__ a_inf, unsigned long long* __restrict__ err) {
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_images * np) return;
    const unsigned long long i = t / np;
    const uint32_t j = (uint32_t)(t % np);
    uint32_t xy[2 * X::N];
    const int rc = srs_decode_point<X, COMPRESSED, VALIDATE, true>(images + i * stride + off[j], xy);
    if (rc >= 0) vfy_agg_report(err, i, fld[j] >> 8, fld[j] & 0xFFu, (uint32_t)rc);
    const bool inf = rc != -1;                                    // (a refused record gets the generator too: the batch is refused anyway)
    if (inf) {
#pragma unroll
        for (int k = 0; k < X::N; k++) { xy[k] = X::GEN_X[k]; xy[X::N + k] = X::GEN_Y[k]; }
    }
    uint32_t* out = bases + t * 2 * X::N;
#pragma unroll
    for (int k = 0; k < 2 * X::N; k++) out[k] = xy[k];
    inf_flags[t] = inf;
    if (j == open_idx || j == open_idx + 1) {                     // the two opening columns also go to the MSM A
        const unsigned long long a = 2 * i + (j - open_idx);
#pragma unroll
        for (int k = 0; k < 2 * X::N; k++) a_bases[a * 2 * X::N + k] = xy[k];
        a_inf[a] = inf;
    }
}

// ---- B -------------------------------------------------------------------------------------------------------------------------------
// 64 challenge bytes (little-endian) mod r, Montgomery: lo + 2^256 hi, each half brought below r by subtraction (2^256 < 6 r)
template <class P>
MZK_D Fp<P> vfy_reduce_halves(Fp<P> lo, Fp<P> hi) {
    while (!ser_below_modulus<P>(lo.l)) sub_limbs<P::N>(lo.l, lo.l, P::MOD);
    while (!ser_below_modulus<P>(hi.l)) sub_limbs<P::N>(hi.l, hi.l, P::MOD);
    return to_mont(lo) + to_mont(to_mont(hi));
}
template <class P>
MZK_D Fp<P> vfy_reduce_challenge(const uint8_t* ch) {
    Fp<P> lo = Fp<P>::zero(), hi = Fp<P>::zero();
#pragma unroll
    for (int s = 0; s < 32; s++) { lo.l[s >> 2] |= (uint32_t)ch[s] << (8 * (s & 3)); hi.l[s >> 2] |= (uint32_t)ch[32 + s] << (8 * (s & 3)); }
    return vfy_reduce_halves<P>(lo, hi);
}
template <class T>
constexpr bool VFY_SOLIDITY = false;                             // the transcript kinds of stage B: Merlin (StandardTranscript) unless stated
template <>
constexpr bool VFY_SOLIDITY<keccak::SolidityTranscript> = true;
template <class T>
MZK_D void vfy_absorb_global(T& t, const uint8_t* __restrict__ p, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) t.absorb_byte(p[i]);
}
template <class T>
MZK_D void vfy_absorb_words(T& t, const uint32_t (&w)[8]) {      // 32 bytes, little-endian (an Fr record)
#pragma unroll
    for (int k = 0; k < 8; k++)
        for (int b = 0; b < 32; b += 8) t.absorb_byte(w[k] >> b);
}
// a G1 record of the image enters the transcript in its COMPRESSED form: as it stands, or rebuilt from an uncompressed record (x's bytes,
// the infinity flag, and "y is the larger" = y > (q - 1) / 2)
template <class X, class T>
MZK_D void vfy_append_g1(T& t, const char* label, uint32_t label_len, const uint8_t* __restrict__ rec, bool compressed) {
    constexpr int B = SerFmt<X>::BYTES;
    constexpr bool BLS = SerFmt<X>::BE;
    t.append_begin(label, label_len, B);
    if (compressed) { vfy_absorb_global(t, rec, B); return; }
    uint32_t yw[X::N];
    ser_read<X>(rec + B, yw);
    const uint32_t f = BLS ? rec[0] : rec[2 * B - 1];
    const bool inf = f & 0x40u;
    yw[X::N - 1] &= BLS ? 0x1FFFFFFFu : 0x3FFFFFFFu;
    bool larger = false, decided = false;
#pragma unroll
    for (int k = X::N - 1; k >= 0; k--) {                        // y > q >> 1
        const uint32_t h = (X::MOD[k] >> 1) | (k + 1 < X::N ? X::MOD[k + 1] << 31 : 0u);
        if (!decided && yw[k] != h) { larger = yw[k] > h; decided = true; }
    }
    larger = larger && !inf;
    for (int s = 0; s < B; s++) {
        uint32_t b = rec[s];
        if (BLS && s == 0) b = (b & 0x1Fu) | 0x80u | (inf ? 0x40u : 0u) | (larger ? 0x20u : 0u);
        if (!BLS && s == B - 1) b = (b & 0x3Fu) | (inf ? 0x40u : 0u) | (larger ? 0x80u : 0u);
        t.absorb_byte(b);
    }
}
// get_and_append_challenge.  The Solidity transcript only records the point (nothing is appended, solidity.rs:59-77): its challenges are
// hashed together at the kernel's end (vfy_store_challenges) and the value returned here is not one
template <class P, class T>
MZK_D Fp<P> vfy_challenge(T& t, const char* label, uint32_t label_len) {
    if constexpr (VFY_SOLIDITY<T>) {
        t.mark();
        return Fp<P>::zero();
    } else {
        uint8_t ch[64];
        t.challenge_bytes(label, label_len, ch, 64);
        const Fp<P> c = vfy_reduce_challenge<P>(ch);
        const Fp<P> v = from_mont(c);
        t.append_begin(label, label_len, 32);
        vfy_absorb_words(t, v.l);
        return c;
    }
}

// A thread's n challenges to out[8 k ..]: Merlin's are in ch; the Solidity transcript hashes its recorded prefixes now, each challenge
// the first 48 bytes of the new state, reduced as the 64 of Merlin with the high 16 zero
template <class P, class T>
MZK_D void vfy_store_challenges(T& t, const Fp<P>* ch, int n, uint32_t* __restrict__ out) {
    if constexpr (VFY_SOLIDITY<T>) {
        t.squeeze_all([&](uint32_t k, const uint64_t (&st)[keccak::STATE_WORDS]) {
            Fp<P> lo = Fp<P>::zero(), hi = Fp<P>::zero();
#pragma unroll
            for (int j = 0; j < 4; j++) { lo.l[2 * j] = (uint32_t)st[j]; lo.l[2 * j + 1] = (uint32_t)(st[j] >> 32); }
#pragma unroll
            for (int j = 0; j < 2; j++) { hi.l[2 * j] = (uint32_t)st[4 + j]; hi.l[2 * j + 1] = (uint32_t)(st[4 + j] >> 32); }
            store_fp<P>(out + k * 8ull, vfy_reduce_halves<P>(lo, hi));
        });
    } else {
        for (int k = 0; k < n; k++) store_fp<P>(out + k * 8ull, ch[k]);
    }
}
// script: the appends of append_vk_and_pub_input up to the public inputs, as items { label_len u8, msg_len u8, label, msg }, n_items of them
// (the Solidity transcript drops the labels and the lengths: it takes the messages alone)
template <class T>
MZK_D const uint8_t* vfy_append_script(T& t, const uint8_t* __restrict__ s, uint32_t n_items) {
    for (uint32_t k = 0; k < n_items; k++) {
        const uint32_t ll = s[0], ml = s[1];
        if constexpr (!VFY_SOLIDITY<T>) {
            t.begin_op(merlin::F_M | merlin::F_A);
            vfy_absorb_global(t, s + 2, ll);
            t.absorb_u32le(ml);
            t.begin_op(merlin::F_A);
        }
        vfy_absorb_global(t, s + 2 + ll, ml);
        s += 2 + ll + ml;
    }
    return s;
}
// A thread's transcript.  Merlin: 25 lanes in LDS (`lanes`), interleaved among the block's threads.  Solidity: a slot of slot_words words in
// device memory, [ state | transcript ], interleaved among the block's 64 threads: word j of thread t at slots[(block * slot_words + j) * 64 + t]
template <class T>
constexpr int VFY_LDS_LANES = VFY_SOLIDITY<T> ? 1 : 25 * VFY_THREADS;
template <class T>
MZK_D void vfy_transcript_init(T& t, uint64_t* lanes, uint64_t* slots, uint32_t slot_words, const char* label, uint32_t label_len) {
    if constexpr (VFY_SOLIDITY<T>) t.init(slots + (unsigned long long)blockIdx.x * slot_words * VFY_THREADS + threadIdx.x, VFY_THREADS, slot_words);
    else t.init(lanes + threadIdx.x, VFY_THREADS, label, label_len);
}
// Proof i: label, its extra message, per position the key's script and the instance's public inputs, then the image's own records
template <class P, class X, class T = merlin::Transcript>
__global__ __launch_bounds__(VFY_THREADS) void vfy_agg_transcript_kernel(const uint8_t* __restrict__ images, unsigned long long K, VfyAggShape sh,
                                                                         const uint8_t* __restrict__ script, const uint32_t* __restrict__ pos_tab,
                                                                         const uint32_t* __restrict__ pub_inputs /* K x total_inputs canonical */,
                                                                         const uint8_t* __restrict__ extra, const unsigned long long* __restrict__ extra_range,
                                                                         uint32_t* __restrict__ challenges, uint64_t* slots, uint32_t slot_words) {
    __shared__ uint64_t lanes[VFY_LDS_LANES<T>];
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const uint8_t* img = images + i * sh.proof_len;
    const uint32_t G = sh.g1_bytes, W = sh.W, m = sh.m;
    const bool cmp = sh.compressed;
    T t;
    vfy_transcript_init(t, lanes, slots, slot_words, VFY_LBL("PlonkProof"));
    if (extra_range && extra_range[2 * i] != ~0ull) {
        const unsigned long long b = extra_range[2 * i], e = extra_range[2 * i + 1];
        t.append_begin(VFY_LBL("extra info"), (uint32_t)(e - b));
        vfy_absorb_global(t, extra + b, (uint32_t)(e - b));
    }
    for (uint32_t j = 0; j < m; j++) {                            // append_vk_and_pub_input, position by position
        const uint32_t p0 = pos_tab[3 * j + 2], p1 = pos_tab[3 * j + 5];
        vfy_append_script(t, script + pos_tab[3 * j], pos_tab[3 * j + 1]);
        for (uint32_t k = p0; k < p1; k++) {
            const uint32_t* w = pub_inputs + (i * sh.total_inputs + k) * 8ull;
            uint32_t v[8];
#pragma unroll
            for (int l = 0; l < 8; l++) v[l] = w[l];
            t.append_begin(VFY_LBL("public input"), 32);
            vfy_absorb_words(t, v);
        }
    }
    Fp<P> ch[7];
    for (uint32_t j = 0; j < m; j++)
        for (uint32_t k = 0; k < W; k++) vfy_append_g1<X>(t, VFY_LBL("witness_poly_comms"), img + sh.wires_off + j * sh.wires_stride + k * G, cmp);
    ch[0] = vfy_challenge<P>(t, VFY_LBL("tau"));
    if (sh.ultra)
        for (uint32_t j = 0; j < m; j++)
            for (uint32_t k = 0; k < 2; k++) vfy_append_g1<X>(t, VFY_LBL("h_poly_comms"), img + sh.plk_off + j * sh.plk_stride + 9 + k * G, cmp);
    ch[1] = vfy_challenge<P>(t, VFY_LBL("beta"));
    ch[2] = vfy_challenge<P>(t, VFY_LBL("gamma"));
    for (uint32_t j = 0; j < m; j++) vfy_append_g1<X>(t, VFY_LBL("perm_poly_comms"), img + sh.prod_off + j * G, cmp);
    if (sh.ultra)
        for (uint32_t j = 0; j < m; j++) vfy_append_g1<X>(t, VFY_LBL("plookup_poly_comms"), img + sh.plk_off + j * sh.plk_stride + 9 + 2 * G, cmp);
    ch[3] = vfy_challenge<P>(t, VFY_LBL("alpha"));
    for (uint32_t k = 0; k < W; k++) vfy_append_g1<X>(t, VFY_LBL("quot_poly_comms"), img + sh.quot_off + k * G, cmp);
    ch[4] = vfy_challenge<P>(t, VFY_LBL("zeta"));
    for (uint32_t j = 0; j < m; j++) {                            // transcript/mod.rs:140-163, instance by instance
        const uint8_t* ev = img + sh.evals_off + j * sh.evals_stride;
        for (uint32_t k = 0; k < W; k++) { t.append_begin(VFY_LBL("wire_evals"), 32); vfy_absorb_global(t, ev + 8 + 32 * k, 32); }
        for (uint32_t k = 0; k + 1 < W; k++) { t.append_begin(VFY_LBL("wire_sigma_evals"), 32); vfy_absorb_global(t, ev + 16 + 32 * (W + k), 32); }
        t.append_begin(VFY_LBL("perm_next_eval"), 32);
        vfy_absorb_global(t, ev + 16 + 32 * (2 * W - 1), 32);
    }
    if (sh.ultra)
        for (uint32_t j = 0; j < m; j++) {                        // transcript/mod.rs:165-202
            const uint8_t* pe = img + sh.plk_off + j * sh.plk_stride + 9 + 3 * G;
            t.append_begin(VFY_LBL("lookup_table_eval"), 32);      vfy_absorb_global(t, pe + 32 * 0, 32);
            t.append_begin(VFY_LBL("h_1_eval"), 32);               vfy_absorb_global(t, pe + 32 * 4, 32);
            t.append_begin(VFY_LBL("prod_next_eval"), 32);         vfy_absorb_global(t, pe + 32 * 6, 32);
            t.append_begin(VFY_LBL("lookup_table_next_eval"), 32); vfy_absorb_global(t, pe + 32 * 7, 32);
            t.append_begin(VFY_LBL("h_1_next_eval"), 32);          vfy_absorb_global(t, pe + 32 * 10, 32);
            t.append_begin(VFY_LBL("h_2_next_eval"), 32);          vfy_absorb_global(t, pe + 32 * 11, 32);
        }
    ch[5] = vfy_challenge<P>(t, VFY_LBL("v"));
    vfy_append_g1<X>(t, VFY_LBL("open_proof"), img + sh.quot_off + W * G, cmp);
    vfy_append_g1<X>(t, VFY_LBL("shifted_open_proof"), img + sh.quot_off + (W + 1) * G, cmp);
    ch[6] = vfy_challenge<P>(t, VFY_LBL("u"));
    vfy_store_challenges<P>(t, ch, 7, challenges + i * 7 * 8ull);
}

// ---- C -------------------------------------------------------------------------------------------------------------------------------
// an Fr record of the image: its range check (stage C makes one pass over an instance's records) and its value
template <class P>
MZK_D void vfy_agg_check_eval(const uint8_t* __restrict__ p, unsigned long long* err, unsigned long long proof, uint32_t inst, uint32_t index) {
    uint32_t a[8];
    fr_read_record(p, a);
    if (!ser_below_modulus<P>(a)) vfy_agg_report(err, proof, inst, VFY_FIELD_EVAL + index, VFY_REASON_NOT_BELOW_R);
}
template <class P>
MZK_D Fp<P> vfy_agg_eval(const uint8_t* __restrict__ p) {
    Fp<P> a;
    fr_read_record(p, a.l);
    return to_mont(a);
}
template <class P>
MZK_D Fp<P> vfy_pow_small(Fp<P> b, uint32_t e) {
    Fp<P> r = Fp<P>::one();
    for (; e; e >>= 1) {
        if (e & 1) r = r * b;
        b = sqr(b);
    }
    return r;
}

// Instance j of proof i.  The type is a template switch, so W and every column index is a constant: each scalar is finished in registers and
// stored once, straight to its place in the proof's two rows (no run-time-indexed row in scratch).  partials: K x m, what instance j adds
// to the proof's aggregated evaluation: sum of e * (its powers of v and u v) - step^j * (its linearisation constant).
template <class P, bool ULTRA>
__global__ __launch_bounds__(VFY_THREADS) void vfy_agg_scalars_kernel(const uint8_t* __restrict__ images, unsigned long long K, VfyAggShape sh,
                                                                      const uint32_t* __restrict__ k_mont /* m x W */, const uint32_t* __restrict__ pos_tab,
                                                                      const uint32_t* __restrict__ pub_inputs, const uint32_t* __restrict__ challenges,
                                                                      uint32_t* __restrict__ key_rows, uint32_t* __restrict__ proof_rows,
                                                                      uint32_t* __restrict__ partials, unsigned long long* __restrict__ err) {
    using F = Fp<P>;
    constexpr uint32_t W = ULTRA ? 6 : 5, NSEL = ULTRA ? 14 : 13, SIG = NSEL, PLK = NSEL + W;
    constexpr uint32_t C_V = 2 * W - 1 + (ULTRA ? 6 : 0), C_U = ULTRA ? 10 : 1;   // commitments one instance opens at zeta / at zeta w (verifier.rs:453-506)
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= K * sh.m) return;
    const unsigned long long i = t / sh.m;
    const uint32_t j = (uint32_t)(t % sh.m), G = sh.g1_bytes;
    const uint8_t* img = images + i * sh.proof_len;
    const F tau = load_fp<P>(challenges + (i * 7 + 0) * 8ull), beta = load_fp<P>(challenges + (i * 7 + 1) * 8ull),
            gamma = load_fp<P>(challenges + (i * 7 + 2) * 8ull), alpha = load_fp<P>(challenges + (i * 7 + 3) * 8ull),
            zeta = load_fp<P>(challenges + (i * 7 + 4) * 8ull), v = load_fp<P>(challenges + (i * 7 + 5) * 8ull),
            u = load_fp<P>(challenges + (i * 7 + 6) * 8ull);
    const uint8_t* ev = img + sh.evals_off + j * sh.evals_stride;
    const uint8_t* pl = img + sh.plk_off + j * sh.plk_stride + 9 + 3 * G;
    // every record's range check first; the values are then read where they are used -- the fifteen Plookup evaluations two or three times
    // each, from cache: held in registers together they are 120 of them
#pragma unroll 1
    for (uint32_t k = 0; k < 2 * W; k++) vfy_agg_check_eval<P>(ev + (k < W ? 8 : 16) + 32 * k, err, i, j, k);
    if constexpr (ULTRA) {
#pragma unroll 1
        for (uint32_t k = 0; k < 15; k++) vfy_agg_check_eval<P>(pl + 32 * k, err, i, j, 2 * W + k);
    }
    F we[W], se[W - 1];
#pragma unroll
    for (uint32_t k = 0; k < W; k++) we[k] = vfy_agg_eval<P>(ev + 8 + 32 * k);
#pragma unroll
    for (uint32_t k = 0; k + 1 < W; k++) se[k] = vfy_agg_eval<P>(ev + 16 + 32 * (W + k));
    const F zn = vfy_agg_eval<P>(ev + 16 + 32 * (2 * W - 1));
    // structs.rs:496-541
    enum { RNG, KEY, DOM, QDOM, H1, QL, PRODN, RNGN, KEYN, DOMN, H1N, H2N, QLN, W3N, W4N };
    const auto pe = [&](uint32_t k) { return vfy_agg_eval<P>(pl + 32 * k); };

    // the domain (verifier.rs:776-788) and PI(zeta) over this instance's inputs (:845-880)
    F w = F::from_const(P::ROOT);
    for (int k = (int)sh.log_n; k < P::TWO_ADICITY; k++) w = sqr(w);
    const F w_inv = inv_safegcd<P>(w), one = F::one(), n_f = from_u64<P>(sh.n);
    F zeta_n = zeta;
    for (uint32_t k = 0; k < sh.log_n; k++) zeta_n = sqr(zeta_n);
    const F vanish = zeta_n - one;
    const F l1 = vanish * inv_safegcd<P>(n_f * (zeta - one));
    const F ln = vanish * w_inv * inv_safegcd<P>(n_f * (zeta - w_inv));
    F pi = F::zero();
    {
        const uint32_t p0 = pos_tab[3 * j + 2], p1 = pos_tab[3 * j + 5];
        const F vn = vanish * inv_safegcd<P>(n_f);
        F g = one;
        for (uint32_t k = p0; k < p1; k++) {
            F val = load_fp<P>(pub_inputs + (i * sh.total_inputs + k) * 8ull);
            if (!ser_below_modulus<P>(val.l)) vfy_agg_report(err, i, j, VFY_FIELD_PUB_INPUT + (k - p0), VFY_REASON_NOT_BELOW_R);
            if (!vanish.is_zero()) pi = pi + vn * g * inv_safegcd<P>(zeta - g) * to_mont(val);
            g = g * w;
        }
    }
    const F a2 = sqr(alpha), a3 = a2 * alpha, a4 = sqr(a2), a5 = a4 * alpha, a6 = a4 * a2;
    const F b1 = one + beta, g_b1 = gamma * b1;
    const F base = vfy_pow_small<P>(ULTRA ? a6 * alpha : a3, j);   // :130-138: alpha^7 | alpha^3 per instance
    // the constant term of the linearisation polynomial (:340-414)
    F lin = pi - a2 * l1;
    {
        F acc = alpha * zn * (gamma + we[W - 1]);
#pragma unroll
        for (uint32_t k = 0; k + 1 < W; k++) acc = acc * (gamma + we[k] + beta * se[k]);
        lin = lin - acc;
    }
    if constexpr (ULTRA) {
        const F h1_e = pe(H1), h2n_e = pe(H2N);
        const F pc = ln * (h1_e - h2n_e - a2) - alpha * l1 - a3 * (zeta - w_inv) * pe(PRODN) * (g_b1 + h1_e + beta * pe(H1N)) * (g_b1 + beta * h2n_e);
        lin = lin + a3 * pc;
    }
    uint32_t* kr = key_rows + (i * sh.nkey + (unsigned long long)j * sh.nkey1) * 8ull;
    uint32_t* pr = proof_rows + (i * sh.np + (unsigned long long)j * (W + 1)) * 8ull;
    uint32_t* pk = proof_rows + (i * sh.np + (unsigned long long)sh.m * (W + 1) + W + 2 + 3ull * j) * 8ull;   // Ultra: h_1, h_2, prod_lookup
    // [D]_1 (:513-652), times step^j
    {
        const F w01 = we[0] * we[1], w23 = we[2] * we[3];
        const auto p5 = [](const F& a) { const F s = sqr(a); return sqr(s) * a; };
        store_fp<P>(kr + 8 * 0, we[0] * base); store_fp<P>(kr + 8 * 1, we[1] * base); store_fp<P>(kr + 8 * 2, we[2] * base); store_fp<P>(kr + 8 * 3, we[3] * base);
        store_fp<P>(kr + 8 * 4, w01 * base); store_fp<P>(kr + 8 * 5, w23 * base);
        store_fp<P>(kr + 8 * 6, p5(we[0]) * base); store_fp<P>(kr + 8 * 7, p5(we[1]) * base); store_fp<P>(kr + 8 * 8, p5(we[2]) * base);
        store_fp<P>(kr + 8 * 9, p5(we[3]) * base);
        store_fp<P>(kr + 8 * 10, neg(we[4]) * base); store_fp<P>(kr + 8 * 11, base); store_fp<P>(kr + 8 * 12, w01 * w23 * we[4] * base);
    }
    F prod_s, plook_s = F::zero(), h2_s = F::zero();
    {
        F coeff = alpha;
#pragma unroll
        for (uint32_t k = 0; k < W; k++) coeff = coeff * (beta * load_fp<P>(k_mont + ((unsigned long long)j * W + k) * 8ull) * zeta + gamma + we[k]);
        prod_s = (coeff + a2 * l1) * base;
        coeff = alpha * beta * zn;
#pragma unroll
        for (uint32_t k = 0; k + 1 < W; k++) coeff = coeff * (beta * se[k] + gamma + we[k]);
        store_fp<P>(kr + 8 * (SIG + W - 1), neg(coeff) * base);
    }
    if constexpr (ULTRA) {
        const F ql_tau = pe(QL) * tau;
        const F merged_lookup_x = we[5] + ql_tau * (pe(QDOM) + tau * (we[0] + tau * (we[1] + tau * we[2])));
        const F table_x = pe(RNG) + ql_tau * (pe(DOM) + tau * (pe(KEY) + tau * (we[3] + tau * we[4])));
        const F table_xw = pe(RNGN) + pe(QLN) * tau * (pe(DOMN) + tau * (pe(KEYN) + tau * (pe(W3N) + tau * pe(W4N))));
        plook_s = (a4 * l1 + a5 * ln + a6 * (zeta - w_inv) * b1 * (gamma + merged_lookup_x) * (g_b1 + table_x + beta * table_xw)) * base;
        h2_s = a6 * (w_inv - zeta) * pe(PRODN) * (g_b1 + pe(H1) + beta * pe(H1N)) * base;
    }
    // this instance's powers of v at zeta and of u v at zeta w (:453-506, :673-733): they start where instance j - 1 stopped
    F share = F::zero(), vb = v * vfy_pow_small<P>(v, j * C_V), uvb = u * vfy_pow_small<P>(v, j * C_U);
    const auto at_zeta = [&](const F& e) { const F p = vb; share = share + e * p; vb = vb * v; return p; };
    const auto at_zeta_omega = [&](const F& e) { const F p = uvb; share = share + e * p; uvb = uvb * v; return p; };
    F wire_s[W];
#pragma unroll
    for (uint32_t k = 0; k < W; k++) wire_s[k] = at_zeta(we[k]);
#pragma unroll
    for (uint32_t k = 0; k + 1 < W; k++) store_fp<P>(kr + 8 * (SIG + k), at_zeta(se[k]));
    store_fp<P>(pr + 8 * W, prod_s + at_zeta_omega(zn));
    if constexpr (ULTRA) {
        const F rng_s = at_zeta(pe(RNG)), key_s = at_zeta(pe(KEY)), h1_s = at_zeta(pe(H1)), ql_s = at_zeta(pe(QL)), dom_s = at_zeta(pe(DOM));
        store_fp<P>(kr + 8 * (PLK + 3), at_zeta(pe(QDOM)));
        store_fp<P>(pk + 8 * 2, plook_s + at_zeta_omega(pe(PRODN)));
        store_fp<P>(kr + 8 * (PLK + 0), rng_s + at_zeta_omega(pe(RNGN)));
        store_fp<P>(kr + 8 * (PLK + 1), key_s + at_zeta_omega(pe(KEYN)));
        store_fp<P>(pk + 8 * 0, h1_s + at_zeta_omega(pe(H1N)));
        store_fp<P>(pk + 8 * 1, h2_s + at_zeta_omega(pe(H2N)));
        store_fp<P>(kr + 8 * 13, ql_s + at_zeta_omega(pe(QLN)));
        wire_s[3] = wire_s[3] + at_zeta_omega(pe(W3N));
        wire_s[4] = wire_s[4] + at_zeta_omega(pe(W4N));
        store_fp<P>(kr + 8 * (PLK + 2), dom_s + at_zeta_omega(pe(DOMN)));
    }
#pragma unroll
    for (uint32_t k = 0; k < W; k++) store_fp<P>(pr + 8 * k, wire_s[k]);
    store_fp<P>(partials + t * 8ull, share - base * lin);
}

// Proof i: eval = the m shares in instance order (a fixed order, no atomics on field elements); the split quotient's scalars (:654-665),
// the two opening proofs' scalars in B (:236-240) and a zero under open_key.g, whose scalar is the finish's.
template <class P>
__global__ __launch_bounds__(VFY_THREADS) void vfy_agg_fold_kernel(unsigned long long K, VfyAggShape sh, const uint32_t* __restrict__ challenges,
                                                                   const uint32_t* __restrict__ partials, uint32_t* __restrict__ key_rows,
                                                                   uint32_t* __restrict__ proof_rows, uint32_t* __restrict__ evals) {
    using F = Fp<P>;
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const F zeta = load_fp<P>(challenges + (i * 7 + 4) * 8ull), u = load_fp<P>(challenges + (i * 7 + 6) * 8ull);
    F w = F::from_const(P::ROOT);
    for (int k = (int)sh.log_n; k < P::TWO_ADICITY; k++) w = sqr(w);
    F zeta_n = zeta;
    for (uint32_t k = 0; k < sh.log_n; k++) zeta_n = sqr(zeta_n);
    const F zeta_n2 = zeta_n * sqr(zeta);
    uint32_t* own = proof_rows + (i * sh.np + (unsigned long long)sh.m * (sh.W + 1)) * 8ull;
    F c = neg(zeta_n - F::one());
    for (uint32_t k = 0; k < sh.W; k++) { store_fp<P>(own + 8 * k, c); c = c * zeta_n2; }
    store_fp<P>(own + 8 * sh.W, zeta);
    store_fp<P>(own + 8 * (sh.W + 1), u * zeta * w);
    F eval = F::zero();
    for (uint32_t j = 0; j < sh.m; j++) eval = eval + load_fp<P>(partials + (i * sh.m + j) * 8ull);
    store_fp<P>(evals + i * 8ull, eval);
    store_fp<P>(key_rows + (i * sh.nkey + sh.nkey - 1) * 8ull, F::zero());
}

// ---- finish --------------------------------------------------------------------------------------------------------------------------
// proof rows *= r_i (0 at a flagged base); A's scalars (r_i, r_i u_i).  NA: A bases per group member -- 2 for a proof (W, W'), 1 for a
// proof link (its opening proof, scalar r_i alone: `challenges` is not read)
template <class P, uint32_t NA = 2>
__global__ __launch_bounds__(256) void vfy_weight_kernel(unsigned long long K, uint32_t np, const uint32_t* __restrict__ weights, const uint32_t* __restrict__ challenges,
                                                         const uint32_t* __restrict__ inf_flags /* K x np */, const uint32_t* __restrict__ a_inf,
                                                         uint32_t* __restrict__ proof_rows, uint32_t* __restrict__ a_scalars) {
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= K * (np + NA)) return;
    const unsigned long long i = t / (np + NA);
    const uint32_t j = (uint32_t)(t % (np + NA));
    const Fp<P> r = load_fp<P>(weights + i * 8ull);
    if (j < np) {
        const Fp<P> s = inf_flags[i * np + j] ? Fp<P>::zero() : r * load_fp<P>(proof_rows + (i * np + j) * 8ull);
        store_fp<P>(proof_rows + (i * np + j) * 8ull, s);
    } else {
        const unsigned long long a = NA * i + (j - np);
        Fp<P> s = (NA == 1 || j == np) ? r : r * load_fp<P>(challenges + (i * 7 + 6) * 8ull);
        if (a_inf[a]) s = Fp<P>::zero();
        store_fp<P>(a_scalars + a * 8ull, s);
    }
}
// column c < nkey - 1: sum_i r_i key_rows[i][c]; the last column (open_key.g): -sum_i r_i evals[i].  One block per column; thread t adds
// rows t, t + 256, .. in order and the 256 partial sums meet in a fixed tree: the same sum on every run, no atomics.
template <class P>
__global__ __launch_bounds__(256) void vfy_colsum_kernel(unsigned long long K, uint32_t nkey, const uint32_t* __restrict__ weights, const uint32_t* __restrict__ key_rows,
                                                         const uint32_t* __restrict__ evals, const uint32_t* __restrict__ key_inf, uint32_t* __restrict__ out) {
    __shared__ uint32_t part[256 * 8];
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const bool last = c == nkey - 1;
    Fp<P> acc = Fp<P>::zero();
    for (unsigned long long i = tid; i < K; i += 256)
        acc = acc + load_fp<P>(weights + i * 8ull) * (last ? load_fp<P>(evals + i * 8ull) : load_fp<P>(key_rows + (i * nkey + c) * 8ull));
#pragma unroll
    for (int k = 0; k < 8; k++) part[tid * 8 + k] = acc.l[k];
    __syncthreads();
    for (uint32_t half = 128; half; half >>= 1) {
        if (tid < half) {
            Fp<P> a, b;
#pragma unroll
            for (int k = 0; k < 8; k++) { a.l[k] = part[tid * 8 + k]; b.l[k] = part[(tid + half) * 8 + k]; }
            a = a + b;
#pragma unroll
            for (int k = 0; k < 8; k++) part[tid * 8 + k] = a.l[k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        Fp<P> s;
#pragma unroll
        for (int k = 0; k < 8; k++) s.l[k] = part[k];
        if (last) s = neg(s);
        if (key_inf[c]) s = Fp<P>::zero();
        store_fp<P>(out + c * 8ull, s);
    }
}

// ---- proof links ---------------------------------------------------------------------------------------------------------------------
// PlonkKzgSnark::verify_link_proof (proof_linking.rs:240-286) for K links, each staged as 4 G1 records back to back: lhs.wires_poly_comms[0],
// rhs.wires_poly_comms[0], quotient_commitment, opening_proof.  A link is the KZG opening of a_1 - a_2 - Z_D(eta) q at eta with value 0
// (univariate_kzg/mod.rs:194-216), so it ends in the pair  A = pi,  B = a_1 - a_2 - Z_D(eta) Q + eta pi  and joins the groups above:
//   key bases    open_key.g alone, scalar zero (NKEY = 1)        proof points  the 4 records, row (1, -1, -Z_D(eta), eta) (NP = 4)
//   A  vfy_decode_kernel          over the 4 records, no opening columns (infinity flagged: two proofs of one circuit link with Q = pi = O)
//   Bl vfy_link_transcript_kernel one thread per link: eta (proof_linking.rs:185-197)
//   Cl vfy_link_vanishing_kernel  one wave per link: Z_D(eta) (:162-176) and the link's row
//   finish                        vfy_weight_kernel<P, 1> (one A base per link), vfy_colsum_kernel over the one key column
template <class P, class X, class T = merlin::Transcript>
__global__ __launch_bounds__(VFY_THREADS) void vfy_link_transcript_kernel(const uint8_t* __restrict__ records, unsigned long long K, uint32_t g1_bytes,
                                                                          uint32_t compressed, uint32_t* __restrict__ eta, uint64_t* slots,
                                                                          uint32_t slot_words) {
    __shared__ uint64_t lanes[VFY_LDS_LANES<T>];
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const uint8_t* rec = records + i * 4ull * g1_bytes;
    const bool cmp = compressed;
    T t;
    vfy_transcript_init(t, lanes, slots, slot_words, VFY_LBL("PlonkLinkingProof"));
    vfy_append_g1<X>(t, VFY_LBL("linking_wire_comms"), rec, cmp);
    vfy_append_g1<X>(t, VFY_LBL("linking_wire_comms"), rec + g1_bytes, cmp);
    vfy_append_g1<X>(t, VFY_LBL("quotient_comm"), rec + 2 * g1_bytes, cmp);
    const Fp<P> ch = vfy_challenge<P>(t, VFY_LBL("eta"));
    vfy_store_challenges<P>(t, &ch, 1, eta + i * 8ull);
}

// Link i, one wave: Z_D(eta) = prod_{k < size} (eta - g^(offset + k)), g the 2^alignment-th root of unity of the NTT (GroupLayout::
// get_domain_generator).  Lane t takes the factors k = t, t + 64, ..: it starts at g^(offset + t) by square-and-multiply (the exponent
// taken mod 2^alignment, the order of g -- an offset + size beyond it wraps, a size beyond it repeats roots, as the reference's loop does)
// and steps by g^64; the 64 partial products meet in LDS by a fixed tree.  Field products are exact, so the order in which the factors
// are multiplied does not change a bit of the result: the same value on every run, and no atomics.  layouts: K x (alignment, offset, size),
// checked on the host (alignment <= TWO_ADICITY, size <= 2^27).  Lane 0 writes Z_D(eta) and the row (1, -1, -Z_D(eta), eta).
template <class P>
__global__ __launch_bounds__(VFY_THREADS) void vfy_link_vanishing_kernel(const unsigned long long* __restrict__ layouts, const uint32_t* __restrict__ eta,
                                                                         uint32_t* __restrict__ vanish, uint32_t* __restrict__ proof_rows) {
    using F = Fp<P>;
    __shared__ uint32_t part[8 * VFY_THREADS];                    // limb-major: lane t's limb k at part[k * 64 + t], no bank conflict
    const unsigned long long i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const unsigned long long alignment = layouts[3 * i], offset = layouts[3 * i + 1], size = layouts[3 * i + 2];
    const F x = load_fp<P>(eta + i * 8ull);
    F g = F::from_const(P::ROOT);
    for (int k = (int)alignment; k < P::TWO_ADICITY; k++) g = sqr(g);
    F root = F::one(), step = g;
    {
        F b = g;
        for (unsigned long long e = (offset + lane) & ((1ull << alignment) - 1); e; e >>= 1) {
            if (e & 1) root = root * b;
            b = sqr(b);
        }
    }
#pragma unroll 1
    for (int k = 0; k < 6; k++) step = sqr(step);                 // g^64
    F acc = F::one();
    for (unsigned long long k = lane; k < size; k += VFY_THREADS) {
        acc = acc * (x - root);
        root = root * step;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) part[k * VFY_THREADS + lane] = acc.l[k];
    __syncthreads();
    for (uint32_t half = VFY_THREADS / 2; half; half >>= 1) {
        if (lane < half) {
            F a, b;
#pragma unroll
            for (int k = 0; k < 8; k++) { a.l[k] = part[k * VFY_THREADS + lane]; b.l[k] = part[k * VFY_THREADS + lane + half]; }
            a = a * b;
#pragma unroll
            for (int k = 0; k < 8; k++) part[k * VFY_THREADS + lane] = a.l[k];
        }
        __syncthreads();
    }
    if (lane == 0) {
        F z;
#pragma unroll
        for (int k = 0; k < 8; k++) z.l[k] = part[k * VFY_THREADS];
        store_fp<P>(vanish + i * 8ull, z);
        uint32_t* row = proof_rows + i * 4 * 8ull;
        store_fp<P>(row, F::one());
        store_fp<P>(row + 8, neg(F::one()));
        store_fp<P>(row + 16, neg(z));
        store_fp<P>(row + 24, x);
    }
}

// ---- KZG openings --------------------------------------------------------------------------------------------------------------------
// UnivariateKzgPCS::verify / batch_verify (univariate_kzg/mod.rs:195-271) for K openings, each staged as 2 G1 records back to back -- the
// commitment C, the opening proof pi -- with its point z and value v as canonical limbs.  e(C - v g + z pi, h) = e(pi, beta_h), so an
// opening ends in the pair  A = pi,  B = C + z pi - v g  and joins the groups above:
//   key bases    open_key.g alone (NKEY = 1), its column the evaluations' (-sum w_i v_i)    proof points  the 2 records, row (1, z) (NP = 2)
//   A  vfy_decode_kernel     over the 2 records, no opening columns (infinity flagged: the zero polynomial commits to O, a constant opens with pi = O)
//   Co vfy_open_rows_kernel  one thread per opening: z, v range-checked against r (fields 2, 3 after the records' 0, 1) and brought to
//                            Montgomery form; the unweighted row (1, z), the evaluation v, z itself, the proof's infinity flag for the MSM A
//   finish                   vfy_weight_kernel<P, 1> (one A base per opening), vfy_colsum_kernel over the one key column
constexpr uint32_t VFY_OPEN_FIELD_POINT = 2, VFY_OPEN_FIELD_VALUE = 3;
template <class P>
__global__ __launch_bounds__(VFY_THREADS) void vfy_open_rows_kernel(unsigned long long K, const uint32_t* __restrict__ points, const uint32_t* __restrict__ values,
                                                                    const uint32_t* __restrict__ inf_flags /* K x 2 */, uint32_t* __restrict__ a_inf,
                                                                    uint32_t* __restrict__ z_mont, uint32_t* __restrict__ key_rows, uint32_t* __restrict__ proof_rows,
                                                                    uint32_t* __restrict__ evals, unsigned long long* __restrict__ err) {
    using F = Fp<P>;
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const F z = load_fp<P>(points + i * 8ull), v = load_fp<P>(values + i * 8ull);
    if (!ser_below_modulus<P>(z.l)) vfy_agg_report(err, i, 0, VFY_OPEN_FIELD_POINT, VFY_REASON_NOT_BELOW_R);
    if (!ser_below_modulus<P>(v.l)) vfy_agg_report(err, i, 0, VFY_OPEN_FIELD_VALUE, VFY_REASON_NOT_BELOW_R);
    const F zm = to_mont(z);
    store_fp<P>(z_mont + i * 8ull, zm);
    store_fp<P>(proof_rows + i * 16ull, F::one());
    store_fp<P>(proof_rows + i * 16ull + 8, zm);
    store_fp<P>(evals + i * 8ull, to_mont(v));
    store_fp<P>(key_rows + i * 8ull, F::zero());                  // open_key.g: its scalar is the evaluations' column sum (vfy_colsum_kernel)
    a_inf[i] = inf_flags[2 * i + 1];
}

}  // namespace mzk
