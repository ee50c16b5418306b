// verifier.hip -- mzk_verifier_*: PlonkKzgSnark::batch_verify for single-instance proofs (snark.rs:141-190, verifier.rs:68-251) and
// verify_batch_proof for aggregated BatchProofs under a tuple of keys (snark.rs:117-138; mzk_verifier_aggregate_*), verify_link_proof for
// proof links under an open key (proof_linking.rs:240-286; mzk_verifier_create_open_key, mzk_verifier_link_*).  The per-proof
// work runs on the device (verifier.cuh: decode, Fiat-Shamir, linearisation scalars), the two MSMs through the variable-base path over a base
// array registered per batch, the two pairings on the host (hostpairing.hpp behind mzk_pairing_product_is_one).
#include "internal.hpp"
#include "hostfp.hpp"
#include "verifier.cuh"

#include <algorithm>
#include <memory>

namespace mzk {
namespace {

struct Verifier {
    int curve = 0, device = -1;                                   // device: the logical device it was created on, where its memory lives
    VfyShape sh{};                                                // (sh.compressed: the mode of the key image and of every proof under it)
    DevOwned key_xy, key_inf, k_mont, script;
    uint32_t n_items = 0, script_len = 0;
    std::vector<uint64_t> h, beta_h;                              // mzk_g2_decode's output
    std::vector<uint64_t> g;                                      // open_key.g as decoded (host copy: an aggregate's tuple compares open keys)
    bool open_only = false;                                       // mzk_verifier_create_open_key: no verifying key, key_xy holds open_key.g alone
    uint32_t g_index() const { return open_only ? 0 : sh.nkey - 1; }   // open_key.g in key_xy / key_inf
};
enum class BatchKind { Proofs, Links };                           // Proofs: single proofs and aggregates (two A bases each); Links: one A base each
struct Batch {
    std::shared_ptr<Verifier> v;                                  // an open batch keeps its verifier alive ...
    std::vector<std::shared_ptr<Verifier>> more;                  // ... and an aggregate batch the verifiers at positions 1 .. m - 1 of its tuple too
    BatchKind kind = BatchKind::Proofs;
    uint64_t K = 0;
    uint32_t np = 0, nkey = 0;                                    // columns of one proof's row and of the key row (an aggregate: NP(m), NKEY(m); links: 4, 1)
    DevOwned images, pub, extra, extra_range, bases, inf, a_bases, a_inf, chal, key_rows, b_scal, evals, a_scal, weights, err;
    DevOwned col_off, col_fld, script, pos_tab, k_mont, partials;   // an aggregate's tables (verifier.cuh)
    DevOwned layouts, vanish;                                     // links: K x (alignment, offset, size); Z_D(eta_i) (eta_i: the first K values of chal)
    std::vector<uint8_t> open_recs;                               // links: the K opening-proof records as staged (mzk_verifier_link_weights)
    bool holds(const std::shared_ptr<Verifier>& x) const { return v == x || std::find(more.begin(), more.end(), x) != more.end(); }
};

// Handles name the logical device of their object (a batch has its verifier's).  g_vfy_lock covers map operations only: a look-up hands out a
// shared_ptr held until the entry point returns, so a destroy or shutdown on another thread takes the handle away and the object goes with its last holder.
std::mutex g_vfy_lock;
std::map<uint64_t, std::shared_ptr<Verifier>> g_verifiers;
std::map<uint64_t, std::shared_ptr<Batch>> g_batches;
uint64_t g_next_verifier = 1, g_next_batch = 1;

uint32_t g1_bytes(int curve, bool compressed) { return (uint32_t)srs_record_bytes(curve, compressed); }

// the layout of a `Proof` image (structs.rs:59-84) under this key's type and mode
void proof_shape(VfyShape& sh) {
    const uint32_t W = sh.W, G = sh.g1_bytes;
    uint32_t o = 8, p = 0;
    for (uint32_t k = 0; k < W; k++, o += G) sh.pt_off[p++] = o;                  // wires_poly_comms
    sh.pt_off[p++] = o; o += G;                                                  // prod_perm_poly_comm
    o += 8;
    for (uint32_t k = 0; k < W; k++, o += G) sh.pt_off[p++] = o;                  // split_quot_poly_comms
    sh.pt_off[p++] = o; o += G;                                                  // opening_proof
    sh.pt_off[p++] = o; o += G;                                                  // shifted_opening_proof
    sh.wires_evals_off = o + 8; o += 8 + 32 * W;
    sh.sigma_evals_off = o + 8; o += 8 + 32 * (W - 1);
    sh.perm_next_off = o; o += 32;
    o += 1;                                                                      // Option<PlookupProof> tag
    if (sh.ultra) {
        o += 8;
        sh.pt_off[p++] = o; o += G;                                              // h_poly_comms
        sh.pt_off[p++] = o; o += G;
        sh.pt_off[p++] = o; o += G;                                              // prod_lookup_poly_comm
        sh.plookup_evals_off = o; o += 32 * 15;
    }
    sh.np = p;
    sh.proof_len = o;
}
const char* proof_point_name(const VfyShape& sh, uint32_t j, std::string& buf) {
    const uint32_t W = sh.W;
    if (j < W) buf = "wires_poly_comms[" + std::to_string(j) + "]";
    else if (j == W) buf = "prod_perm_poly_comm";
    else if (j < 2 * W + 1) buf = "split_quot_poly_comms[" + std::to_string(j - W - 1) + "]";
    else if (j == 2 * W + 1) buf = "opening_proof";
    else if (j == 2 * W + 2) buf = "shifted_opening_proof";
    else if (j < 2 * W + 5) buf = "plookup_proof.h_poly_comms[" + std::to_string(j - 2 * W - 3) + "]";
    else buf = "plookup_proof.prod_lookup_poly_comm";
    return buf.c_str();
}
const char* proof_eval_name(const VfyShape& sh, uint32_t e, std::string& buf) {
    static const char* const PLOOKUP[15] = {"range_table_eval", "key_table_eval", "table_dom_sep_eval", "q_dom_sep_eval", "h_1_eval", "q_lookup_eval",
                                            "prod_next_eval", "range_table_next_eval", "key_table_next_eval", "table_dom_sep_next_eval", "h_1_next_eval",
                                            "h_2_next_eval", "q_lookup_next_eval", "w_3_next_eval", "w_4_next_eval"};
    const uint32_t W = sh.W;
    if (e < W) buf = "wires_evals[" + std::to_string(e) + "]";
    else if (e < 2 * W - 1) buf = "wire_sigma_evals[" + std::to_string(e - W) + "]";
    else if (e == 2 * W - 1) buf = "perm_next_eval";
    else buf = std::string("plookup_proof.") + PLOOKUP[(e - 2 * W) % 15];
    return buf.c_str();
}
const char* reason_text(uint32_t reason) { return reason == VFY_REASON_NOT_BELOW_R ? "not below the modulus" : srs_bad_reason((int)reason); }

template <class X>
void launch_decode(bool compressed, bool validate, const uint8_t* images, uint64_t n_images, const VfyPoints& pts, uint32_t* bases, uint32_t* inf, uint32_t* a_bases,
                   uint32_t* a_inf, unsigned long long* err) {
    const dim3 grid((unsigned)((n_images * pts.n + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
    if (compressed) {
        if (validate) hipLaunchKernelGGL((vfy_decode_kernel<X, true, true>), grid, block, 0, nullptr, images, (unsigned long long)n_images, pts, bases, inf, a_bases, a_inf, err);
        else hipLaunchKernelGGL((vfy_decode_kernel<X, true, false>), grid, block, 0, nullptr, images, (unsigned long long)n_images, pts, bases, inf, a_bases, a_inf, err);
    } else {
        if (validate) hipLaunchKernelGGL((vfy_decode_kernel<X, false, true>), grid, block, 0, nullptr, images, (unsigned long long)n_images, pts, bases, inf, a_bases, a_inf, err);
        else hipLaunchKernelGGL((vfy_decode_kernel<X, false, false>), grid, block, 0, nullptr, images, (unsigned long long)n_images, pts, bases, inf, a_bases, a_inf, err);
    }
}
void decode_points(int curve, bool compressed, bool validate, const uint8_t* images, uint64_t n_images, const VfyPoints& pts, uint32_t* bases, uint32_t* inf,
                   uint32_t* a_bases, uint32_t* a_inf, unsigned long long* err) {
    if (curve == MZK_CURVE_BLS12_381) launch_decode<BlsFqX>(compressed, validate, images, n_images, pts, bases, inf, a_bases, a_inf, err);
    else launch_decode<BnFqX>(compressed, validate, images, n_images, pts, bases, inf, a_bases, a_inf, err);
}

void script_item(std::vector<uint8_t>& s, uint32_t& n_items, const char* label, const uint8_t* msg, size_t len) {
    const size_t ll = std::strlen(label);
    s.push_back((uint8_t)ll);
    s.push_back((uint8_t)len);
    s.insert(s.end(), label, label + ll);
    s.insert(s.end(), msg, msg + len);
    n_items++;
}
template <class FrP>
bool fr_to_mont_host(const uint8_t* rec32, uint64_t* out) {      // false: not below r
    Fp64<FrP> a, r2;
    std::memcpy(a.l, rec32, 32);
    if (Fp64<FrP>::geq_mod(a.l)) return false;
    for (int i = 0; i < 4; i++) r2.l[i] = Fp64<FrP>::c64(FrP::R2, i);
    a = a * r2;
    std::memcpy(out, a.l, 32);
    return true;
}
template <class FqP>
void fq_negate_host(uint64_t* y) {
    Fp64<FqP> a;
    std::memcpy(a.l, y, sizeof a.l);
    a = neg(a);
    std::memcpy(y, a.l, sizeof a.l);
}

std::shared_ptr<Verifier> find_verifier(uint64_t h) {
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    auto it = g_verifiers.find(h);
    if (it == g_verifiers.end()) { set_error("unknown verifier handle"); return nullptr; }
    return it->second;
}
std::shared_ptr<Batch> find_batch(uint64_t h, bool consume = false) {
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    auto it = g_batches.find(h);
    if (it == g_batches.end()) { set_error("unknown batch handle"); return nullptr; }
    std::shared_ptr<Batch> b = it->second;
    if (consume) g_batches.erase(it);
    return b;
}
// An entry point that touches the device runs on the device its handle names (context bits that name no initialised context: an unknown handle).
// The guard is declared BEFORE the shared_ptr, so a last reference drops -- and frees device memory -- while that device is still bound.
int32_t guard_status(const DeviceGuard& g) {
    if (g.rc == MZK_ERR_NOT_INIT) { set_error("unknown handle"); return MZK_ERR_BAD_HANDLE; }
    return g.rc;
}
#define ON_DEVICE_OF(h, obj, find)       \
    DeviceGuard guard_(handle_ctx(h));   \
    MZK_TRY(guard_status(guard_));       \
    const auto obj = find(h);            \
    if (!obj) return MZK_ERR_BAD_HANDLE

int32_t verifier_create(int32_t curve, int device, const uint8_t* vk, uint64_t len, uint32_t flags, uint64_t* out_handle) {
    const bool compressed = flags & MZK_SER_COMPRESSED, validate = flags & MZK_SER_VALIDATE;
    mzk_key_layout_t lay;
    MZK_TRY(mzk_key_layout(curve, vk, len, (flags & MZK_SER_COMPRESSED) | MZK_KEY_VK_ONLY, &lay));
    if (lay.is_merged) { set_error("merged verifying keys are not supported"); return MZK_ERR_UNSUPPORTED; }
    if (len >= (1ull << 31)) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    auto v = std::make_shared<Verifier>();
    v->curve = curve, v->device = device;
    VfyShape& sh = v->sh;
    sh.W = lay.num_wire_types, sh.nsel = lay.num_selectors, sh.ultra = lay.has_plookup_vk, sh.n = lay.domain_size, sh.num_inputs = (uint32_t)lay.num_inputs;
    if (lay.num_inputs > lay.domain_size) { set_error("num_inputs: larger than the domain"); return MZK_ERR_ENCODING; }
    for (sh.log_n = 0; (1ull << sh.log_n) < sh.n; sh.log_n++) {}
    sh.compressed = compressed, sh.g1_bytes = g1_bytes(curve, compressed);
    sh.nkey = sh.nsel + sh.W + (sh.ultra ? 4 : 0) + 1;
    proof_shape(sh);
    const uint32_t G = sh.g1_bytes, nkey = sh.nkey, fqw = fq_words(curve);
    // the key's commitments, decoded on the device; infinity is a normal value here (an unused selector commits to nothing)
    VfyPoints pts{};
    pts.n = nkey, pts.stride = (uint32_t)len, pts.open_idx = -1;
    uint32_t p = 0;
    std::vector<std::string> names;
    for (uint32_t j = 0; j < sh.nsel; j++) { pts.off[p++] = (uint32_t)(lay.selector_comms_off + j * G); names.push_back("selector_comms[" + std::to_string(j) + "]"); }
    for (uint32_t j = 0; j < sh.W; j++) { pts.off[p++] = (uint32_t)(lay.sigma_comms_off + j * G); names.push_back("sigma_comms[" + std::to_string(j) + "]"); }
    static const char* const PLK[4] = {"range_table_comm", "key_table_comm", "table_dom_sep_comm", "q_dom_sep_comm"};
    if (sh.ultra)
        for (uint32_t j = 0; j < 4; j++) { pts.off[p++] = (uint32_t)(lay.plookup_comms_off + j * G); names.push_back(std::string("plookup_vk.") + PLK[j]); }
    pts.off[p++] = (uint32_t)lay.g_off;
    names.push_back("open_key.g");
    DevOwned image, err;
    MZK_TRY(image.alloc(len));
    MZK_TRY(err.alloc(8));
    MZK_TRY(v->key_xy.alloc((size_t)nkey * 2 * fqw * 4));
    MZK_TRY(v->key_inf.alloc((size_t)nkey * 4));
    HIP_TRY(hipMemcpy(image.p, vk, len, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(err.p, 0xFF, 8));
    decode_points(curve, compressed, validate, image.as<uint8_t>(), 1, pts, v->key_xy.as<uint32_t>(), v->key_inf.as<uint32_t>(), nullptr, nullptr,
                  err.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpy(&bad, err.p, 8, hipMemcpyDeviceToHost));
    if (bad != ~0ull) {
        set_error("vk." + names[(bad >> 8) & 0xFFFFFF] + ": " + reason_text((uint32_t)(bad & 0xFF)));
        return MZK_ERR_ENCODING;
    }
    // the byte script of append_vk_and_pub_input (transcript/mod.rs:45-104), commitments in their compressed form
    std::vector<uint64_t> xy((size_t)nkey * 2 * fqw / 2);
    std::vector<uint32_t> inf(nkey);
    HIP_TRY(hipMemcpy(xy.data(), v->key_xy.p, (size_t)nkey * 2 * fqw * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(inf.data(), v->key_inf.p, (size_t)nkey * 4, hipMemcpyDeviceToHost));
    for (uint32_t j = 0; j < nkey; j++)
        if (inf[j]) std::memset(xy.data() + (size_t)j * fqw, 0, (size_t)fqw * 8);       // (0, 0): the encoder's infinity
    const uint32_t GC = g1_bytes(curve, true);
    std::vector<uint8_t> recs((size_t)nkey * GC), script;
    MZK_TRY(mzk_ctx_g1_encode(curve, xy.data(), nkey, MZK_SER_COMPRESSED, recs.data()));
    const uint32_t bits = curve == MZK_CURVE_BLS12_381 ? BlsFr::BITS : BnFr::BITS;
    const uint64_t n64 = sh.n, ni64 = lay.num_inputs;
    script_item(script, v->n_items, "field size in bits", reinterpret_cast<const uint8_t*>(&bits), 4);
    script_item(script, v->n_items, "domain size", reinterpret_cast<const uint8_t*>(&n64), 8);
    script_item(script, v->n_items, "input size", reinterpret_cast<const uint8_t*>(&ni64), 8);
    std::vector<uint64_t> k_mont(4 * sh.W);
    for (uint32_t j = 0; j < sh.W; j++) {
        const uint8_t* rec = vk + lay.k_off + 32 * j;
        const bool ok = curve == MZK_CURVE_BLS12_381 ? fr_to_mont_host<BlsFr>(rec, &k_mont[4 * j]) : fr_to_mont_host<BnFr>(rec, &k_mont[4 * j]);
        if (!ok) { set_error("vk.k[" + std::to_string(j) + "]: not below the modulus"); return MZK_ERR_ENCODING; }
        script_item(script, v->n_items, "wire subsets separators", rec, 32);
    }
    for (uint32_t j = 0; j < sh.nsel; j++) script_item(script, v->n_items, "selector commitments", &recs[(size_t)j * GC], GC);
    for (uint32_t j = 0; j < sh.W; j++) script_item(script, v->n_items, "sigma commitments", &recs[(size_t)(sh.nsel + j) * GC], GC);
    v->script_len = (uint32_t)script.size();
    v->g.assign(xy.begin() + (size_t)(nkey - 1) * fqw, xy.begin() + (size_t)nkey * fqw);
    MZK_TRY(v->script.alloc(script.size()));
    MZK_TRY(v->k_mont.alloc(k_mont.size() * 8));
    HIP_TRY(hipMemcpy(v->script.p, script.data(), script.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v->k_mont.p, k_mont.data(), k_mont.size() * 8, hipMemcpyHostToDevice));
    // h, beta_h: decoded on the host, where the pairing runs
    v->h.resize(4 * fqw / 2);
    v->beta_h.resize(4 * fqw / 2);
    if (mzk_g2_decode(curve, vk + lay.h_off, flags & (MZK_SER_COMPRESSED | MZK_SER_VALIDATE), v->h.data()) != MZK_OK) {
        set_error(std::string("vk.open_key.h: ") + mzk_last_error());
        return MZK_ERR_ENCODING;
    }
    if (mzk_g2_decode(curve, vk + lay.beta_h_off, flags & (MZK_SER_COMPRESSED | MZK_SER_VALIDATE), v->beta_h.data()) != MZK_OK) {
        set_error(std::string("vk.open_key.beta_h: ") + mzk_last_error());
        return MZK_ERR_ENCODING;
    }
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    *out_handle = handle_make(device, g_next_verifier++);
    g_verifiers[*out_handle] = std::move(v);
    return MZK_OK;
}

// the container of proof i on the host: Vec counts and the Option tag against the key's type
bool proof_container_ok(const VfyShape& sh, const uint8_t* img, std::string& why) {
    const auto count = [&](uint32_t off) { uint64_t c; std::memcpy(&c, img + off, 8); return c; };
    const auto expect = [&](const char* field, uint32_t off, uint64_t want) {
        if (count(off) == want) return true;
        why = std::string(field) + ".len: " + std::to_string(count(off)) + ", expected " + std::to_string(want);
        return false;
    };
    const uint32_t W = sh.W, G = sh.g1_bytes;
    if (!expect("wires_poly_comms", 0, W) || !expect("split_quot_poly_comms", sh.pt_off[W] + G, W) || !expect("wires_evals", sh.wires_evals_off - 8, W) ||
        !expect("wire_sigma_evals", sh.sigma_evals_off - 8, W - 1))
        return false;
    const uint8_t tag = img[sh.perm_next_off + 32];
    if (tag != (sh.ultra ? 1 : 0)) {
        why = tag > 1 ? "plookup_proof: invalid Option tag" : sh.ultra ? "plookup_proof: absent under an UltraPlonk key" : "plookup_proof: present under a TurboPlonk key";
        return false;
    }
    return !sh.ultra || expect("plookup_proof.h_poly_comms", sh.perm_next_off + 33, 2);
}

// Stage B under MZK_TRANSCRIPT_SOLIDITY keeps each transcript in a slot of device memory (verifier.cuh, vfy_transcript_init): the 64 bytes of
// the state, at most `transcript_bytes` of transcript and the recorded challenge points, for every thread of the ceil(K / 64) blocks.
uint64_t longest_extra(const uint64_t* extra_ranges, uint64_t K) {
    uint64_t longest = 0;
    if (extra_ranges)
        for (uint64_t i = 0; i < K; i++)
            if (extra_ranges[2 * i] != ~0ull) longest = std::max(longest, extra_ranges[2 * i + 1] - extra_ranges[2 * i]);
    return longest;
}
int32_t alloc_slots(DevOwned& slots, uint64_t K, uint64_t transcript_bytes, uint32_t& slot_words) {
    slot_words = keccak::SolidityTranscript::slot_words(transcript_bytes);
    return slots.alloc((K + VFY_THREADS - 1) / VFY_THREADS * VFY_THREADS * slot_words * 8);
}

int32_t batch_begin(const std::shared_ptr<Verifier>& vp, const uint8_t* proofs, uint64_t proof_len, uint64_t K, const uint64_t* pub, const uint8_t* extra,
                    const uint64_t* extra_ranges, const uint64_t* challenges, uint32_t flags, uint64_t* out_batch, uint64_t* out_u, uint64_t* out_bad) {
    const Verifier& v = *vp;
    const VfyShape& sh = v.sh;
    if (out_bad) *out_bad = ~0ull;
    if (proof_len != sh.proof_len) {
        if (out_bad) *out_bad = 0;
        set_error("proof 0: length: " + std::to_string(proof_len) + " bytes, expected " + std::to_string(sh.proof_len) + " under this key");
        return MZK_ERR_ENCODING;
    }
    for (uint64_t i = 0; i < K; i++) {
        std::string why;
        if (!proof_container_ok(sh, proofs + i * proof_len, why)) {
            if (out_bad) *out_bad = i;
            set_error("proof " + std::to_string(i) + ": " + why);
            return MZK_ERR_ENCODING;
        }
    }
    uint64_t extra_len = 0;
    if (extra_ranges)
        for (uint64_t i = 0; i < K; i++) {
            const uint64_t b = extra_ranges[2 * i], e = extra_ranges[2 * i + 1];
            if (b == ~0ull) continue;
            if (e < b || e - b >= (1ull << 31) || !extra) { set_error("bad extra message range"); return MZK_ERR_INVALID_ARG; }
            extra_len = std::max(extra_len, e);
        }
    const int curve = v.curve;
    const uint32_t np = sh.np, nkey = sh.nkey, fqw = fq_words(curve);
    const size_t pt_bytes = (size_t)2 * fqw * 4, n_bases = nkey + K * np;
    auto b = std::make_shared<Batch>();                               // (a failure below frees it here, under the caller's guard)
    b->v = vp, b->K = K, b->np = np, b->nkey = nkey;
    MZK_TRY(b->images.alloc(K * proof_len));
    MZK_TRY(b->pub.alloc(K * sh.num_inputs * 32));
    MZK_TRY(b->extra.alloc(extra_len));
    MZK_TRY(b->extra_range.alloc(K * 16));
    MZK_TRY(b->bases.alloc(n_bases * pt_bytes));
    MZK_TRY(b->inf.alloc(n_bases * 4));
    MZK_TRY(b->a_bases.alloc(2 * K * pt_bytes));
    MZK_TRY(b->a_inf.alloc(2 * K * 4));
    MZK_TRY(b->chal.alloc(K * 7 * 32));
    MZK_TRY(b->key_rows.alloc(K * nkey * 32));
    MZK_TRY(b->b_scal.alloc(n_bases * 32));
    MZK_TRY(b->evals.alloc(K * 32));
    MZK_TRY(b->a_scal.alloc(2 * K * 32));
    MZK_TRY(b->weights.alloc(K * 32));
    MZK_TRY(b->err.alloc(8));
    HIP_TRY(hipMemcpy(b->images.p, proofs, K * proof_len, hipMemcpyHostToDevice));           // the K images in one copy
    if (sh.num_inputs) HIP_TRY(hipMemcpy(b->pub.p, pub, K * sh.num_inputs * 32, hipMemcpyHostToDevice));
    if (extra_len) HIP_TRY(hipMemcpy(b->extra.p, extra, extra_len, hipMemcpyHostToDevice));
    if (extra_ranges) HIP_TRY(hipMemcpy(b->extra_range.p, extra_ranges, K * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b->err.p, 0xFF, 8));
    HIP_TRY(hipMemcpy(b->bases.p, v.key_xy.p, nkey * pt_bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(b->inf.p, v.key_inf.p, nkey * 4, hipMemcpyDeviceToDevice));
    unsigned long long* err = b->err.as<unsigned long long>();
    // A
    VfyPoints pts{};
    pts.n = np, pts.stride = sh.proof_len, pts.open_idx = (int32_t)(2 * sh.W + 1);
    for (uint32_t j = 0; j < np; j++) pts.off[j] = sh.pt_off[j];
    decode_points(curve, sh.compressed, flags & MZK_SER_VALIDATE, b->images.as<uint8_t>(), K, pts, b->bases.as<uint32_t>() + (size_t)nkey * 2 * fqw,
                  b->inf.as<uint32_t>() + nkey, b->a_bases.as<uint32_t>(), b->a_inf.as<uint32_t>(), err);
    HIP_TRY(hipGetLastError());
    // B, or the caller's challenges
    const dim3 grid((unsigned)((K + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
    DevOwned slots;                                                   // Solidity: the transcripts' memory, freed when the stages are through
    if (challenges) {
        HIP_TRY(hipMemcpy(b->chal.p, challenges, K * 7 * 32, hipMemcpyHostToDevice));
    } else {
        ProfScope ps("vfy_transcript", nullptr, v.device);
        const unsigned long long* ranges = extra_ranges ? b->extra_range.as<unsigned long long>() : nullptr;
        const bool solidity = flags & MZK_TRANSCRIPT_SOLIDITY;
        uint32_t slot_words = 0;
        // (the script's length bounds its messages; the proof's own: np commitments in compressed form, 2 W (+ 6) evaluations)
        if (solidity)
            MZK_TRY(alloc_slots(slots, K, longest_extra(extra_ranges, K) + v.script_len + 32ull * sh.num_inputs + (uint64_t)np * g1_bytes(curve, true) +
                                              32ull * (2 * sh.W + 6), slot_words));
#define MZK_VFY_TRANSCRIPT(Fr, FqX, T)                                                                                                                        \
    hipLaunchKernelGGL((vfy_transcript_kernel<Fr, FqX, T>), grid, block, 0, nullptr, b->images.as<uint8_t>(), (unsigned long long)K, sh, v.script.as<uint8_t>(), \
                       v.n_items, b->pub.as<uint32_t>(), b->extra.as<uint8_t>(), ranges, b->chal.as<uint32_t>(), err, slots.as<uint64_t>(), slot_words)
        if (curve == MZK_CURVE_BLS12_381) {
            if (solidity) MZK_VFY_TRANSCRIPT(BlsFr, BlsFqX, keccak::SolidityTranscript);
            else MZK_VFY_TRANSCRIPT(BlsFr, BlsFqX, merlin::Transcript);
        } else {
            if (solidity) MZK_VFY_TRANSCRIPT(BnFr, BnFqX, keccak::SolidityTranscript);
            else MZK_VFY_TRANSCRIPT(BnFr, BnFqX, merlin::Transcript);
        }
#undef MZK_VFY_TRANSCRIPT
        HIP_TRY(hipGetLastError());
    }
    // C
    uint32_t* proof_rows = b->b_scal.as<uint32_t>() + (size_t)nkey * 8;
    if (curve == MZK_CURVE_BLS12_381)
        hipLaunchKernelGGL((vfy_scalars_kernel<BlsFr>), grid, block, 0, nullptr, b->images.as<uint8_t>(), (unsigned long long)K, sh, v.k_mont.as<uint32_t>(),
                           b->pub.as<uint32_t>(), b->chal.as<uint32_t>(), b->key_rows.as<uint32_t>(), proof_rows, b->evals.as<uint32_t>(), err);
    else
        hipLaunchKernelGGL((vfy_scalars_kernel<BnFr>), grid, block, 0, nullptr, b->images.as<uint8_t>(), (unsigned long long)K, sh, v.k_mont.as<uint32_t>(),
                           b->pub.as<uint32_t>(), b->chal.as<uint32_t>(), b->key_rows.as<uint32_t>(), proof_rows, b->evals.as<uint32_t>(), err);
    HIP_TRY(hipGetLastError());
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpy(&bad, b->err.p, 8, hipMemcpyDeviceToHost));                             // (synchronises the three stages)
    if (bad != ~0ull) {
        const uint64_t i = bad >> 32;
        const uint32_t field = (uint32_t)(bad >> 8) & 0xFFFFFF, reason = (uint32_t)bad & 0xFF;
        std::string buf;
        const std::string name = field >= VFY_FIELD_PUB_INPUT ? "public_input[" + std::to_string(field - VFY_FIELD_PUB_INPUT) + "]"
                                 : field >= VFY_FIELD_EVAL    ? proof_eval_name(sh, field - VFY_FIELD_EVAL, buf)
                                                              : proof_point_name(sh, field, buf);
        if (out_bad) *out_bad = i;
        set_error("proof " + std::to_string(i) + ": " + name + ": " + reason_text(reason));
        return MZK_ERR_ENCODING;
    }
    if (out_u) HIP_TRY(hipMemcpy2D(out_u, 32, b->chal.as<uint8_t>() + 6 * 32, 7 * 32, 32, K, hipMemcpyDeviceToHost));
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    *out_batch = handle_make(v.device, g_next_batch++);
    g_batches[*out_batch] = std::move(b);
    return MZK_OK;
}

template <class Fr, uint32_t NA>
void launch_finish(const Batch& b, uint64_t K, uint32_t np, uint32_t nkey) {
    uint32_t* proof_rows = b.b_scal.as<uint32_t>() + (size_t)nkey * 8;
    const dim3 wgrid((unsigned)((K * (np + NA) + 255) / 256));
    hipLaunchKernelGGL((vfy_weight_kernel<Fr, NA>), wgrid, dim3(256), 0, nullptr, (unsigned long long)K, np, b.weights.as<uint32_t>(), b.chal.as<uint32_t>(),
                       b.inf.as<uint32_t>() + nkey, b.a_inf.as<uint32_t>(), proof_rows, b.a_scal.as<uint32_t>());
    hipLaunchKernelGGL((vfy_colsum_kernel<Fr>), dim3(nkey), dim3(256), 0, nullptr, (unsigned long long)K, nkey, b.weights.as<uint32_t>(), b.key_rows.as<uint32_t>(),
                       b.evals.as<uint32_t>(), b.inf.as<uint32_t>(), b.b_scal.as<uint32_t>());
}
int32_t batch_finish(Batch& b, const uint64_t* weights, uint64_t* out_A, uint64_t* out_B) {
    const Verifier& v = *b.v;
    const uint64_t K = b.K;
    const uint32_t np = b.np, nkey = b.nkey;
    HIP_TRY(hipMemcpy(b.weights.p, weights, K * 32, hipMemcpyHostToDevice));
    const bool links = b.kind == BatchKind::Links;
    if (v.curve == MZK_CURVE_BLS12_381) links ? launch_finish<BlsFr, 1>(b, K, np, nkey) : launch_finish<BlsFr, 2>(b, K, np, nkey);
    else links ? launch_finish<BnFr, 1>(b, K, np, nkey) : launch_finish<BnFr, 2>(b, K, np, nkey);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    // the two MSMs of verifier.rs:217-247 through the variable-base path (links: A over the K opening proofs)
    const struct { void* bases; void* scalars; uint64_t n; uint64_t* out; } jobs[2] = {{b.a_bases.p, b.a_scal.p, links ? K : 2 * K, out_A},
                                                                                      {b.bases.p, b.b_scal.p, nkey + K * np, out_B}};
    for (const auto& j : jobs) {
        uint64_t srs = 0;
        MZK_TRY(mzk_srs_register_dev(v.curve, j.bases, j.n, &srs, nullptr));
        const int32_t rc = mzk_msm_dev(srs, 0, j.scalars, j.n, 1, j.out, nullptr);
        (void)hipDeviceSynchronize();
        (void)mzk_srs_release(srs);
        MZK_TRY(rc);
    }
    return MZK_OK;
}

// ---- aggregated BatchProofs (structs.rs:266-291) -------------------------------------------------------------------------------------------
void batch_proof_layout(uint32_t G, bool ultra, uint32_t m, mzk_batch_proof_layout_t& L) {
    const uint32_t W = ultra ? 6 : 5;
    L = mzk_batch_proof_layout_t{};
    L.m = m, L.num_wire_types = W, L.ultra = ultra, L.g1_record_bytes = G;
    uint64_t o = 8;                                                                  // wires_poly_comms_vec
    for (uint32_t j = 0; j < m; j++) { L.wires_off[j] = o + 8; o += 8 + (uint64_t)W * G; }
    o += 8;                                                                          // prod_perm_poly_comms_vec
    for (uint32_t j = 0; j < m; j++, o += G) L.prod_perm_off[j] = o;
    o += 8;                                                                          // poly_evals_vec
    for (uint32_t j = 0; j < m; j++) {
        L.wires_evals_off[j] = o + 8; o += 8 + 32 * W;
        L.sigma_evals_off[j] = o + 8; o += 8 + 32 * (W - 1);
        L.perm_next_off[j] = o; o += 32;
    }
    o += 8;                                                                          // plookup_proofs_vec
    for (uint32_t j = 0; j < m; j++) {
        L.plookup_tag_off[j] = o; o += 1;
        if (!ultra) continue;
        L.h_off[j] = o + 8; o += 8 + 2 * G;
        L.prod_lookup_off[j] = o; o += G;
        L.plookup_evals_off[j] = o; o += 32 * 15;
    }
    L.split_quot_off = o + 8; o += 8 + (uint64_t)W * G;
    L.opening_off = o; o += G;
    L.shifted_opening_off = o; o += G;
    L.total_len = o;
}
// the container of one image against the layout, in image order: `inst` is the instance the defect belongs to (m: the whole proof)
bool batch_proof_container_ok(const mzk_batch_proof_layout_t& L, const uint8_t* img, uint64_t len, uint32_t& inst, std::string& why) {
    const uint32_t m = L.m, W = L.num_wire_types;
    inst = m;
    if (len != L.total_len) {
        why = "length: " + std::to_string(len) + " bytes, expected " + std::to_string(L.total_len) + " under these keys";
        return false;
    }
    const auto expect = [&](const char* field, uint64_t off, uint64_t want, uint32_t j) {
        uint64_t c;
        std::memcpy(&c, img + off, 8);
        if (c == want) return true;
        inst = j;
        why = std::string(field) + ".len: " + std::to_string(c) + ", expected " + std::to_string(want);
        return false;
    };
    if (!expect("wires_poly_comms_vec", 0, m, m)) return false;
    for (uint32_t j = 0; j < m; j++)
        if (!expect("wires_poly_comms", L.wires_off[j] - 8, W, j)) return false;
    if (!expect("prod_perm_poly_comms_vec", L.prod_perm_off[0] - 8, m, m) || !expect("poly_evals_vec", L.wires_evals_off[0] - 16, m, m)) return false;
    for (uint32_t j = 0; j < m; j++)
        if (!expect("wires_evals", L.wires_evals_off[j] - 8, W, j) || !expect("wire_sigma_evals", L.sigma_evals_off[j] - 8, W - 1, j)) return false;
    if (!expect("plookup_proofs_vec", L.plookup_tag_off[0] - 8, m, m)) return false;
    for (uint32_t j = 0; j < m; j++) {
        const uint8_t tag = img[L.plookup_tag_off[j]];
        if (tag != (L.ultra ? 1 : 0)) {
            inst = j;
            why = tag > 1 ? "plookup_proof: invalid Option tag" : L.ultra ? "plookup_proof: absent under an UltraPlonk key" : "plookup_proof: present under a TurboPlonk key";
            return false;
        }
        if (L.ultra && !expect("plookup_proof.h_poly_comms", L.h_off[j] - 8, 2, j)) return false;
    }
    return expect("split_quot_poly_comms", L.split_quot_off - 8, W, m);
}

// the tuple on the host: one curve, device, mode, domain, open key and type; fills the shape the kernels take
int32_t tuple_shape(const std::vector<std::shared_ptr<Verifier>>& vs, VfyAggShape& ag, mzk_batch_proof_layout_t& L) {
    const Verifier& v0 = *vs[0];
    const uint32_t m = (uint32_t)vs.size();
    uint64_t total_inputs = 0;
    for (uint32_t j = 0; j < m; j++) {
        const Verifier& v = *vs[j];
        if (v.open_only) { set_error("the verifier holds no verifying key"); return MZK_ERR_INVALID_ARG; }
        if (v.curve != v0.curve) { set_error("the verification keys are of different curves"); return MZK_ERR_INVALID_ARG; }
        if (v.device != v0.device) { set_error("the verifiers live on different devices"); return MZK_ERR_INVALID_ARG; }
        if (v.sh.compressed != v0.sh.compressed) { set_error("the verification keys have different image modes"); return MZK_ERR_INVALID_ARG; }
        if (v.sh.n != v0.sh.n) { set_error("the domain size of the " + std::to_string(j) + "-th verification key is different"); return MZK_ERR_INVALID_ARG; }
        if (v.g != v0.g || v.h != v0.h || v.beta_h != v0.beta_h) { set_error("the verification keys have different open keys"); return MZK_ERR_INVALID_ARG; }
        if (v.sh.ultra != v0.sh.ultra) { set_error("a tuple of TurboPlonk and UltraPlonk keys is not supported"); return MZK_ERR_UNSUPPORTED; }
        total_inputs += v.sh.num_inputs;
    }
    if (total_inputs >= (1ull << 28)) { set_error("too many public inputs"); return MZK_ERR_UNSUPPORTED; }
    const VfyShape& s = v0.sh;
    batch_proof_layout(s.g1_bytes, s.ultra, m, L);
    ag = VfyAggShape{};
    ag.m = m, ag.W = s.W, ag.nsel = s.nsel, ag.ultra = s.ultra, ag.log_n = s.log_n, ag.compressed = s.compressed, ag.g1_bytes = s.g1_bytes, ag.n = s.n;
    ag.nkey1 = s.nkey - 1, ag.nkey = m * ag.nkey1 + 1;
    ag.np = m * (s.W + 1) + s.W + 2 + (s.ultra ? 3 * m : 0);
    ag.proof_len = (uint32_t)L.total_len, ag.total_inputs = (uint32_t)total_inputs;
    ag.wires_off = (uint32_t)L.wires_off[0], ag.wires_stride = 8 + s.W * s.g1_bytes;
    ag.prod_off = (uint32_t)L.prod_perm_off[0];
    ag.evals_off = (uint32_t)L.wires_evals_off[0] - 8, ag.evals_stride = 16 + 32 * 2 * s.W;
    ag.plk_off = (uint32_t)L.plookup_tag_off[0], ag.plk_stride = s.ultra ? 9 + 3 * s.g1_bytes + 32 * 15 : 1;
    ag.quot_off = (uint32_t)L.split_quot_off;
    return MZK_OK;
}
int32_t find_tuple(const uint64_t* handles, uint32_t m, std::vector<std::shared_ptr<Verifier>>& vs) {
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    for (uint32_t j = 0; j < m; j++) {
        auto it = g_verifiers.find(handles[j]);
        if (it == g_verifiers.end()) { set_error("unknown verifier handle"); return MZK_ERR_BAD_HANDLE; }
        vs.push_back(it->second);
    }
    return MZK_OK;
}
int32_t tuple_args(const uint64_t* handles, uint32_t m) {
    if (!handles || !m) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    if (m > MZK_VERIFIER_MAX_INSTANCES) { set_error("more than " + std::to_string(MZK_VERIFIER_MAX_INSTANCES) + " instances in one aggregate"); return MZK_ERR_UNSUPPORTED; }
    return MZK_OK;
}
std::string agg_field_name(const VfyAggShape& ag, uint32_t inst, uint32_t field) {
    const uint32_t W = ag.W;
    std::string buf;
    if (field >= VFY_FIELD_PUB_INPUT) return "public_input[" + std::to_string(field - VFY_FIELD_PUB_INPUT) + "]";
    if (field >= VFY_FIELD_EVAL) {
        VfyShape one{};
        one.W = W;
        return proof_eval_name(one, field - VFY_FIELD_EVAL, buf);
    }
    if (inst == ag.m) return field < W ? "split_quot_poly_comms[" + std::to_string(field) + "]" : field == W ? "opening_proof" : "shifted_opening_proof";
    if (field < W) return "wires_poly_comms[" + std::to_string(field) + "]";
    if (field == W) return "prod_perm_poly_comm";
    return field < W + 3 ? "plookup_proof.h_poly_comms[" + std::to_string(field - W - 1) + "]" : "plookup_proof.prod_lookup_poly_comm";
}

template <class X>
void launch_agg_decode(bool compressed, bool validate, const uint8_t* images, uint64_t K, const VfyAggShape& ag, const Batch& b, uint32_t* bases, uint32_t* inf,
                       unsigned long long* err) {
    const dim3 grid((unsigned)((K * ag.np + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
    const uint32_t open_idx = ag.m * (ag.W + 1) + ag.W;
#define MZK_AGG_DECODE(C, V)                                                                                                                             \
    hipLaunchKernelGGL((vfy_agg_decode_kernel<X, C, V>), grid, block, 0, nullptr, images, (unsigned long long)K, ag.np, ag.proof_len, b.col_off.as<uint32_t>(), \
                       b.col_fld.as<uint32_t>(), open_idx, bases, inf, b.a_bases.as<uint32_t>(), b.a_inf.as<uint32_t>(), err)
    if (compressed) {
        if (validate) MZK_AGG_DECODE(true, true);
        else MZK_AGG_DECODE(true, false);
    } else {
        if (validate) MZK_AGG_DECODE(false, true);
        else MZK_AGG_DECODE(false, false);
    }
#undef MZK_AGG_DECODE
}
template <class Fr>
void launch_agg_scalars(const Batch& b, uint64_t K, const VfyAggShape& ag, uint32_t* proof_rows, unsigned long long* err) {
    const dim3 grid((unsigned)((K * ag.m + VFY_THREADS - 1) / VFY_THREADS)), fold((unsigned)((K + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
    if (ag.ultra)
        hipLaunchKernelGGL((vfy_agg_scalars_kernel<Fr, true>), grid, block, 0, nullptr, b.images.as<uint8_t>(), (unsigned long long)K, ag, b.k_mont.as<uint32_t>(),
                           b.pos_tab.as<uint32_t>(), b.pub.as<uint32_t>(), b.chal.as<uint32_t>(), b.key_rows.as<uint32_t>(), proof_rows, b.partials.as<uint32_t>(), err);
    else
        hipLaunchKernelGGL((vfy_agg_scalars_kernel<Fr, false>), grid, block, 0, nullptr, b.images.as<uint8_t>(), (unsigned long long)K, ag, b.k_mont.as<uint32_t>(),
                           b.pos_tab.as<uint32_t>(), b.pub.as<uint32_t>(), b.chal.as<uint32_t>(), b.key_rows.as<uint32_t>(), proof_rows, b.partials.as<uint32_t>(), err);
    hipLaunchKernelGGL((vfy_agg_fold_kernel<Fr>), fold, block, 0, nullptr, (unsigned long long)K, ag, b.chal.as<uint32_t>(), b.partials.as<uint32_t>(),
                       b.key_rows.as<uint32_t>(), proof_rows, b.evals.as<uint32_t>());
}

int32_t aggregate_begin(const std::vector<std::shared_ptr<Verifier>>& vs, const uint8_t* proofs, uint64_t proof_len, uint64_t K, const uint64_t* pub,
                        const uint8_t* extra, const uint64_t* extra_ranges, const uint64_t* challenges, uint32_t flags, uint64_t* out_batch, uint64_t* out_u,
                        uint64_t* out_bad) {
    VfyAggShape ag;
    mzk_batch_proof_layout_t L;
    MZK_TRY(tuple_shape(vs, ag, L));
    if (ag.total_inputs && !pub) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    const Verifier& v0 = *vs[0];
    const uint32_t m = ag.m, W = ag.W, np = ag.np, nkey = ag.nkey, nkey1 = ag.nkey1;
    if (out_bad) *out_bad = ~0ull;
    for (uint64_t i = 0; i < K; i++) {                               // (a wrong length is every proof's: reported for proof 0, as the single-proof path does)
        std::string why;
        uint32_t inst;
        if (!batch_proof_container_ok(L, proofs + i * proof_len, proof_len, inst, why)) {
            if (out_bad) *out_bad = i;
            set_error("proof " + std::to_string(i) + ": instance " + std::to_string(inst) + ": " + why);
            return MZK_ERR_ENCODING;
        }
    }
    uint64_t extra_len = 0;
    if (extra_ranges)
        for (uint64_t i = 0; i < K; i++) {
            const uint64_t b = extra_ranges[2 * i], e = extra_ranges[2 * i + 1];
            if (b == ~0ull) continue;
            if (e < b || e - b >= (1ull << 31) || !extra) { set_error("bad extra message range"); return MZK_ERR_INVALID_ARG; }
            extra_len = std::max(extra_len, e);
        }
    // the tables: columns of stage A (offset; instance << 8 | field), the positions' scripts and public-input ranges
    std::vector<uint32_t> col_off, col_fld, pos_tab;
    const auto col = [&](uint64_t off, uint32_t inst, uint32_t field) { col_off.push_back((uint32_t)off); col_fld.push_back(inst << 8 | field); };
    for (uint32_t j = 0; j < m; j++) {
        for (uint32_t k = 0; k < W; k++) col(L.wires_off[j] + (uint64_t)k * ag.g1_bytes, j, k);
        col(L.prod_perm_off[j], j, W);
    }
    for (uint32_t k = 0; k < W; k++) col(L.split_quot_off + (uint64_t)k * ag.g1_bytes, m, k);
    col(L.opening_off, m, W);
    col(L.shifted_opening_off, m, W + 1);
    if (ag.ultra)
        for (uint32_t j = 0; j < m; j++) {
            col(L.h_off[j], j, W + 1);
            col(L.h_off[j] + ag.g1_bytes, j, W + 2);
            col(L.prod_lookup_off[j], j, W + 3);
        }
    uint32_t script_len = 0, inputs = 0;
    for (uint32_t j = 0; j < m; j++) {
        pos_tab.insert(pos_tab.end(), {script_len, vs[j]->n_items, inputs});
        script_len += vs[j]->script_len, inputs += vs[j]->sh.num_inputs;
    }
    pos_tab.insert(pos_tab.end(), {script_len, 0u, inputs});
    const int curve = v0.curve;
    const uint32_t fqw = fq_words(curve);
    const size_t pt_bytes = (size_t)2 * fqw * 4, n_bases = nkey + K * np;
    auto b = std::make_shared<Batch>();                               // (a failure below frees it here, under the caller's guard)
    b->v = vs[0], b->more.assign(vs.begin() + 1, vs.end()), b->K = K, b->np = np, b->nkey = nkey;
    MZK_TRY(b->images.alloc(K * proof_len));
    MZK_TRY(b->pub.alloc(K * ag.total_inputs * 32));
    MZK_TRY(b->extra.alloc(extra_len));
    MZK_TRY(b->extra_range.alloc(K * 16));
    MZK_TRY(b->bases.alloc(n_bases * pt_bytes));
    MZK_TRY(b->inf.alloc(n_bases * 4));
    MZK_TRY(b->a_bases.alloc(2 * K * pt_bytes));
    MZK_TRY(b->a_inf.alloc(2 * K * 4));
    MZK_TRY(b->chal.alloc(K * 7 * 32));
    MZK_TRY(b->key_rows.alloc(K * nkey * 32));
    MZK_TRY(b->b_scal.alloc(n_bases * 32));
    MZK_TRY(b->evals.alloc(K * 32));
    MZK_TRY(b->a_scal.alloc(2 * K * 32));
    MZK_TRY(b->weights.alloc(K * 32));
    MZK_TRY(b->err.alloc(8));
    MZK_TRY(b->col_off.alloc((size_t)np * 4));
    MZK_TRY(b->col_fld.alloc((size_t)np * 4));
    MZK_TRY(b->script.alloc(script_len));
    MZK_TRY(b->pos_tab.alloc(pos_tab.size() * 4));
    MZK_TRY(b->k_mont.alloc((size_t)m * W * 32));
    MZK_TRY(b->partials.alloc(K * m * 32));
    HIP_TRY(hipMemcpy(b->images.p, proofs, K * proof_len, hipMemcpyHostToDevice));
    if (ag.total_inputs) HIP_TRY(hipMemcpy(b->pub.p, pub, K * ag.total_inputs * 32, hipMemcpyHostToDevice));
    if (extra_len) HIP_TRY(hipMemcpy(b->extra.p, extra, extra_len, hipMemcpyHostToDevice));
    if (extra_ranges) HIP_TRY(hipMemcpy(b->extra_range.p, extra_ranges, K * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->col_off.p, col_off.data(), (size_t)np * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->col_fld.p, col_fld.data(), (size_t)np * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->pos_tab.p, pos_tab.data(), pos_tab.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b->err.p, 0xFF, 8));
    for (uint32_t j = 0; j < m; j++) {                                // per POSITION: a repeated key repeats its block, its script and its k
        const Verifier& v = *vs[j];
        HIP_TRY(hipMemcpyAsync(b->bases.as<uint8_t>() + (size_t)j * nkey1 * pt_bytes, v.key_xy.p, nkey1 * pt_bytes, hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(b->inf.as<uint32_t>() + (size_t)j * nkey1, v.key_inf.p, nkey1 * 4, hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(b->script.as<uint8_t>() + pos_tab[3 * j], v.script.p, v.script_len, hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(b->k_mont.as<uint8_t>() + (size_t)j * W * 32, v.k_mont.p, (size_t)W * 32, hipMemcpyDeviceToDevice, nullptr));
    }
    HIP_TRY(hipMemcpyAsync(b->bases.as<uint8_t>() + (size_t)(nkey - 1) * pt_bytes, v0.key_xy.as<uint8_t>() + (size_t)nkey1 * pt_bytes, pt_bytes, hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(b->inf.as<uint32_t>() + (nkey - 1), v0.key_inf.as<uint32_t>() + nkey1, 4, hipMemcpyDeviceToDevice, nullptr));
    unsigned long long* err = b->err.as<unsigned long long>();
    uint32_t* bases = b->bases.as<uint32_t>() + (size_t)nkey * 2 * fqw;
    uint32_t* proof_rows = b->b_scal.as<uint32_t>() + (size_t)nkey * 8;
    const bool validate = flags & MZK_SER_VALIDATE;
    if (curve == MZK_CURVE_BLS12_381) launch_agg_decode<BlsFqX>(ag.compressed, validate, b->images.as<uint8_t>(), K, ag, *b, bases, b->inf.as<uint32_t>() + nkey, err);
    else launch_agg_decode<BnFqX>(ag.compressed, validate, b->images.as<uint8_t>(), K, ag, *b, bases, b->inf.as<uint32_t>() + nkey, err);
    HIP_TRY(hipGetLastError());
    DevOwned slots;                                                   // Solidity: the transcripts' memory, freed when the stages are through
    if (challenges) {
        HIP_TRY(hipMemcpy(b->chal.p, challenges, K * 7 * 32, hipMemcpyHostToDevice));
    } else {
        const dim3 grid((unsigned)((K + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
        const unsigned long long* ranges = extra_ranges ? b->extra_range.as<unsigned long long>() : nullptr;
        const bool solidity = flags & MZK_TRANSCRIPT_SOLIDITY;
        uint32_t slot_words = 0;
        if (solidity)
            MZK_TRY(alloc_slots(slots, K, longest_extra(extra_ranges, K) + script_len + 32ull * ag.total_inputs + (uint64_t)np * g1_bytes(curve, true) +
                                              32ull * m * (2 * W + 6), slot_words));
#define MZK_VFY_TRANSCRIPT(Fr, FqX, T)                                                                                                                           \
    hipLaunchKernelGGL((vfy_agg_transcript_kernel<Fr, FqX, T>), grid, block, 0, nullptr, b->images.as<uint8_t>(), (unsigned long long)K, ag, b->script.as<uint8_t>(), \
                       b->pos_tab.as<uint32_t>(), b->pub.as<uint32_t>(), b->extra.as<uint8_t>(), ranges, b->chal.as<uint32_t>(), slots.as<uint64_t>(), slot_words)
        if (curve == MZK_CURVE_BLS12_381) {
            if (solidity) MZK_VFY_TRANSCRIPT(BlsFr, BlsFqX, keccak::SolidityTranscript);
            else MZK_VFY_TRANSCRIPT(BlsFr, BlsFqX, merlin::Transcript);
        } else {
            if (solidity) MZK_VFY_TRANSCRIPT(BnFr, BnFqX, keccak::SolidityTranscript);
            else MZK_VFY_TRANSCRIPT(BnFr, BnFqX, merlin::Transcript);
        }
#undef MZK_VFY_TRANSCRIPT
        HIP_TRY(hipGetLastError());
    }
    if (curve == MZK_CURVE_BLS12_381) launch_agg_scalars<BlsFr>(*b, K, ag, proof_rows, err);
    else launch_agg_scalars<BnFr>(*b, K, ag, proof_rows, err);
    HIP_TRY(hipGetLastError());
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpy(&bad, b->err.p, 8, hipMemcpyDeviceToHost));                             // (synchronises the stages)
    if (bad != ~0ull) {
        const uint64_t i = bad >> 40;
        const uint32_t inst = (uint32_t)(bad >> 33) & 0x7F, field = (uint32_t)(bad >> 4) & 0x1FFFFFFF, reason = (uint32_t)bad & 0xF;
        if (out_bad) *out_bad = i;
        set_error("proof " + std::to_string(i) + ": instance " + std::to_string(inst) + ": " + agg_field_name(ag, inst, field) + ": " + reason_text(reason));
        return MZK_ERR_ENCODING;
    }
    if (out_u) HIP_TRY(hipMemcpy2D(out_u, 32, b->chal.as<uint8_t>() + 6 * 32, 7 * 32, 32, K, hipMemcpyDeviceToHost));
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    *out_batch = handle_make(v0.device, g_next_batch++);
    g_batches[*out_batch] = std::move(b);
    return MZK_OK;
}

// ---- proof links (proof_linking.rs:240-286; verifier.cuh "proof links") ---------------------------------------------------------------------
int32_t open_key_create(int32_t curve, int device, const uint8_t* g_bytes, const uint8_t* h_bytes, const uint8_t* beta_h_bytes, uint32_t flags, uint64_t* out_handle) {
    const bool compressed = flags & MZK_SER_COMPRESSED, validate = flags & MZK_SER_VALIDATE;
    auto v = std::make_shared<Verifier>();
    v->curve = curve, v->device = device, v->open_only = true;
    v->sh.compressed = compressed, v->sh.g1_bytes = g1_bytes(curve, compressed);       // np = nkey = proof_len = 0: no verifying key
    const uint32_t G = v->sh.g1_bytes, fqw = fq_words(curve);
    VfyPoints pts{};
    pts.n = 1, pts.stride = G, pts.open_idx = -1;
    DevOwned image, err;
    MZK_TRY(image.alloc(G));
    MZK_TRY(err.alloc(8));
    MZK_TRY(v->key_xy.alloc((size_t)2 * fqw * 4));
    MZK_TRY(v->key_inf.alloc(4));
    HIP_TRY(hipMemcpy(image.p, g_bytes, G, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(err.p, 0xFF, 8));
    decode_points(curve, compressed, validate, image.as<uint8_t>(), 1, pts, v->key_xy.as<uint32_t>(), v->key_inf.as<uint32_t>(), nullptr, nullptr,
                  err.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpy(&bad, err.p, 8, hipMemcpyDeviceToHost));
    if (bad != ~0ull) {
        set_error(std::string("open_key.g: ") + reason_text((uint32_t)(bad & 0xFF)));
        return MZK_ERR_ENCODING;
    }
    uint32_t inf = 0;
    v->g.resize((size_t)2 * fqw / 2);
    HIP_TRY(hipMemcpy(v->g.data(), v->key_xy.p, (size_t)2 * fqw * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&inf, v->key_inf.p, 4, hipMemcpyDeviceToHost));
    if (inf) std::fill(v->g.begin(), v->g.end(), 0);                 // (0, 0): as verifier_create keeps a flagged g
    v->h.resize(4 * fqw / 2);
    v->beta_h.resize(4 * fqw / 2);
    if (mzk_g2_decode(curve, h_bytes, flags & (MZK_SER_COMPRESSED | MZK_SER_VALIDATE), v->h.data()) != MZK_OK) {
        set_error(std::string("open_key.h: ") + mzk_last_error());
        return MZK_ERR_ENCODING;
    }
    if (mzk_g2_decode(curve, beta_h_bytes, flags & (MZK_SER_COMPRESSED | MZK_SER_VALIDATE), v->beta_h.data()) != MZK_OK) {
        set_error(std::string("open_key.beta_h: ") + mzk_last_error());
        return MZK_ERR_ENCODING;
    }
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    *out_handle = handle_make(device, g_next_verifier++);
    g_verifiers[*out_handle] = std::move(v);
    return MZK_OK;
}

constexpr uint64_t LINK_MAX_SIZE = 1ull << 27;                       // the largest domain of the library (mzk_ntt)
const char* const LINK_FIELDS[4] = {"lhs.wires_poly_comms[0]", "rhs.wires_poly_comms[0]", "quotient_commitment", "opening_proof"};

int32_t link_begin(const std::shared_ptr<Verifier>& vp, const uint8_t* records, uint64_t K, const uint64_t* layouts, const uint64_t* eta, uint32_t flags,
                   uint64_t* out_batch, uint64_t* out_eta, uint64_t* out_bad) {
    const Verifier& v = *vp;
    const int curve = v.curve;
    if (out_bad) *out_bad = ~0ull;
    const uint64_t two_adicity = curve == MZK_CURVE_BLS12_381 ? BlsFr::TWO_ADICITY : BnFr::TWO_ADICITY;
    for (uint64_t i = 0; i < K; i++) {                                 // (offset + size beyond 2^alignment: accepted, the roots wrap or repeat)
        if (layouts[3 * i] > two_adicity) {
            set_error("link " + std::to_string(i) + ": alignment " + std::to_string(layouts[3 * i]) + " is above the field's two-adicity " + std::to_string(two_adicity));
            return MZK_ERR_INVALID_ARG;
        }
        if (layouts[3 * i + 2] > LINK_MAX_SIZE) {
            set_error("link " + std::to_string(i) + ": size " + std::to_string(layouts[3 * i + 2]) + " is above 2^27");
            return MZK_ERR_UNSUPPORTED;
        }
    }
    const uint32_t G = v.sh.g1_bytes, np = 4, nkey = 1, fqw = fq_words(curve);
    const size_t pt_bytes = (size_t)2 * fqw * 4, n_bases = nkey + K * np;
    auto b = std::make_shared<Batch>();                               // (a failure below frees it here, under the caller's guard)
    b->v = vp, b->kind = BatchKind::Links, b->K = K, b->np = np, b->nkey = nkey;
    b->open_recs.resize(K * G);
    for (uint64_t i = 0; i < K; i++) std::memcpy(&b->open_recs[i * G], records + (i * 4 + 3) * G, G);
    MZK_TRY(b->images.alloc(K * 4 * G));
    MZK_TRY(b->layouts.alloc(K * 24));
    MZK_TRY(b->bases.alloc(n_bases * pt_bytes));
    MZK_TRY(b->inf.alloc(n_bases * 4));
    MZK_TRY(b->a_bases.alloc(K * pt_bytes));
    MZK_TRY(b->a_inf.alloc(K * 4));
    MZK_TRY(b->chal.alloc(K * 32));
    MZK_TRY(b->vanish.alloc(K * 32));
    MZK_TRY(b->key_rows.alloc(K * nkey * 32));
    MZK_TRY(b->b_scal.alloc(n_bases * 32));
    MZK_TRY(b->evals.alloc(K * 32));
    MZK_TRY(b->a_scal.alloc(K * 32));
    MZK_TRY(b->weights.alloc(K * 32));
    MZK_TRY(b->err.alloc(8));
    HIP_TRY(hipMemcpy(b->images.p, records, K * 4 * G, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->layouts.p, layouts, K * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b->err.p, 0xFF, 8));
    HIP_TRY(hipMemset(b->key_rows.p, 0, K * nkey * 32));              // open_key.g: scalar zero, and the opened value is 0
    HIP_TRY(hipMemset(b->evals.p, 0, K * 32));
    HIP_TRY(hipMemcpy(b->bases.p, v.key_xy.as<uint8_t>() + (size_t)v.g_index() * pt_bytes, pt_bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(b->inf.p, v.key_inf.as<uint32_t>() + v.g_index(), 4, hipMemcpyDeviceToDevice));
    unsigned long long* err = b->err.as<unsigned long long>();
    // A: the existing decoder over a 4-record image; the opening proofs (column 3) are then gathered as the bases of the MSM A
    VfyPoints pts{};
    pts.n = np, pts.stride = 4 * G, pts.open_idx = -1;
    for (uint32_t j = 0; j < np; j++) pts.off[j] = j * G;
    uint8_t* own_bases = b->bases.as<uint8_t>() + (size_t)nkey * pt_bytes;
    decode_points(curve, v.sh.compressed, flags & MZK_SER_VALIDATE, b->images.as<uint8_t>(), K, pts, reinterpret_cast<uint32_t*>(own_bases), b->inf.as<uint32_t>() + nkey,
                  nullptr, nullptr, err);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(b->a_bases.p, pt_bytes, own_bases + 3 * pt_bytes, 4 * pt_bytes, pt_bytes, K, hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpy2DAsync(b->a_inf.p, 4, b->inf.as<uint32_t>() + nkey + 3, 16, 4, K, hipMemcpyDeviceToDevice, nullptr));
    // Bl, or the caller's eta
    DevOwned slots;                                                   // Solidity: the transcripts' memory, freed when the stages are through
    if (eta) {
        HIP_TRY(hipMemcpy(b->chal.p, eta, K * 32, hipMemcpyHostToDevice));
    } else {
        ProfScope ps("vfy_link_transcript", nullptr, v.device);
        const dim3 grid((unsigned)((K + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
        const bool solidity = flags & MZK_TRANSCRIPT_SOLIDITY;
        uint32_t slot_words = 0;
        if (solidity) MZK_TRY(alloc_slots(slots, K, 3ull * g1_bytes(curve, true), slot_words));
#define MZK_VFY_TRANSCRIPT(Fr, FqX, T)                                                                                                                      \
    hipLaunchKernelGGL((vfy_link_transcript_kernel<Fr, FqX, T>), grid, block, 0, nullptr, b->images.as<uint8_t>(), (unsigned long long)K, G, v.sh.compressed, \
                       b->chal.as<uint32_t>(), slots.as<uint64_t>(), slot_words)
        if (curve == MZK_CURVE_BLS12_381) {
            if (solidity) MZK_VFY_TRANSCRIPT(BlsFr, BlsFqX, keccak::SolidityTranscript);
            else MZK_VFY_TRANSCRIPT(BlsFr, BlsFqX, merlin::Transcript);
        } else {
            if (solidity) MZK_VFY_TRANSCRIPT(BnFr, BnFqX, keccak::SolidityTranscript);
            else MZK_VFY_TRANSCRIPT(BnFr, BnFqX, merlin::Transcript);
        }
#undef MZK_VFY_TRANSCRIPT
        HIP_TRY(hipGetLastError());
    }
    // Cl
    {
        ProfScope ps("vfy_link_vanishing", nullptr, v.device);
        uint32_t* proof_rows = b->b_scal.as<uint32_t>() + (size_t)nkey * 8;
        const dim3 grid((unsigned)K), block(VFY_THREADS);
        if (curve == MZK_CURVE_BLS12_381)
            hipLaunchKernelGGL((vfy_link_vanishing_kernel<BlsFr>), grid, block, 0, nullptr, b->layouts.as<unsigned long long>(), b->chal.as<uint32_t>(),
                               b->vanish.as<uint32_t>(), proof_rows);
        else
            hipLaunchKernelGGL((vfy_link_vanishing_kernel<BnFr>), grid, block, 0, nullptr, b->layouts.as<unsigned long long>(), b->chal.as<uint32_t>(),
                               b->vanish.as<uint32_t>(), proof_rows);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpy(&bad, b->err.p, 8, hipMemcpyDeviceToHost));                             // (synchronises the stages)
    if (bad != ~0ull) {
        const uint64_t i = bad >> 32;
        if (out_bad) *out_bad = i;
        set_error("link " + std::to_string(i) + ": " + LINK_FIELDS[(bad >> 8) & 3] + ": " + reason_text((uint32_t)bad & 0xFF));
        return MZK_ERR_ENCODING;
    }
    if (out_eta) HIP_TRY(hipMemcpy(out_eta, b->chal.p, K * 32, hipMemcpyDeviceToHost));
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    *out_batch = handle_make(v.device, g_next_batch++);
    g_batches[*out_batch] = std::move(b);
    return MZK_OK;
}

// 64 challenge bytes mod r, Montgomery: vfy_reduce_challenge on the host (lo + 2^256 hi, each half below r by subtraction: 2^256 < 6 r)
template <class FrP>
Fp64<FrP> reduce_challenge_host(const uint8_t* ch) {
    using F = Fp64<FrP>;
    F lo = F::zero(), hi = F::zero(), r2;
    for (int s = 0; s < 32; s++) { lo.l[s >> 3] |= (uint64_t)ch[s] << (8 * (s & 7)); hi.l[s >> 3] |= (uint64_t)ch[32 + s] << (8 * (s & 7)); }
    for (int i = 0; i < 4; i++) r2.l[i] = F::c64(FrP::R2, i);
    while (F::geq_mod(lo.l)) F::sub_mod(lo.l);
    while (F::geq_mod(hi.l)) F::sub_mod(hi.l);
    return lo * r2 + (hi * r2) * r2;
}
template <class FrP>
void fr_record_host(const uint64_t* mont, uint8_t* rec) {            // Montgomery -> 32 B little-endian canonical
    Fp64<FrP> a;
    std::memcpy(a.l, mont, sizeof a.l);
    const auto c = h64::canonical(a);
    for (int s = 0; s < 32; s++) rec[s] = (uint8_t)(c[s >> 3] >> (8 * (s & 7)));
}
// The weights of a link batch: s^(i + 1), s drawn from r (when the links stand beside Plonk groups), every eta_i and every opening-proof
// record.  eta_i binds a_1, a_2 and Q but not pi_i, so the pi_i enter too; no weight is 1 beside a Plonk group, whose first proof has r^0.
template <class FrP>
void link_weights_t(const uint64_t* r_mont, const uint64_t* eta, const std::vector<uint8_t>& open_recs, uint64_t K, uint64_t* out) {
    using F = Fp64<FrP>;
    if (K == 1 && !r_mont) { const F one = F::one(); std::memcpy(out, one.l, sizeof one.l); return; }
    const uint32_t G = (uint32_t)(open_recs.size() / K);
    uint64_t lanes[25];
    uint8_t rec[32], ch[64];
    merlin::Transcript t;
    t.init(lanes, 1, "batch verify links", 18);
    if (r_mont) { fr_record_host<FrP>(r_mont, rec); t.append_message("r", 1, rec, 32); }
    for (uint64_t i = 0; i < K; i++) { fr_record_host<FrP>(eta + 4 * i, rec); t.append_message("eta", 3, rec, 32); }
    for (uint64_t i = 0; i < K; i++) t.append_message("opening_proof", 13, &open_recs[i * G], G);
    t.challenge_bytes("s", 1, ch, 64);
    const F s = reduce_challenge_host<FrP>(ch);
    F w = s;
    for (uint64_t i = 0; i < K; i++, w = w * s) std::memcpy(out + 4 * i, w.l, sizeof w.l);
}

}  // namespace

void verifier_release_all() {                                         // mzk_shutdown, per context (bound): its handles go; what a call in flight holds goes with that call
    const int logical = cur().logical;
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    for (auto it = g_batches.begin(); it != g_batches.end();) it = handle_ctx(it->first) == logical ? g_batches.erase(it) : std::next(it);
    for (auto it = g_verifiers.begin(); it != g_verifiers.end();) it = handle_ctx(it->first) == logical ? g_verifiers.erase(it) : std::next(it);
}

}  // namespace mzk

using namespace mzk;

extern "C" int32_t mzk_verifier_create(int32_t curve_id, const uint8_t* vk_bytes, uint64_t len, uint32_t flags, uint64_t* out_handle) {
    if (!valid_curve(curve_id) || !vk_bytes || !out_handle || (flags & ~(MZK_SER_COMPRESSED | MZK_SER_VALIDATE))) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    int32_t device;                                                   // the calling thread's context: a key image names no device
    MZK_TRY(mzk_get_device(&device));
    return verifier_create(curve_id, device, vk_bytes, len, flags, out_handle);
}

extern "C" int32_t mzk_verifier_destroy(uint64_t verifier) {
    DeviceGuard guard(handle_ctx(verifier));
    MZK_TRY(guard_status(guard));
    std::shared_ptr<Verifier> v;                                      // (the last reference, unless a call in flight holds one: the buffers go with it)
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    auto it = g_verifiers.find(verifier);
    if (it == g_verifiers.end()) { set_error("unknown verifier handle"); return MZK_ERR_BAD_HANDLE; }
    for (const auto& kv : g_batches)
        if (kv.second->holds(it->second)) { set_error("the verifier has an open batch"); return MZK_ERR_INVALID_ARG; }
    v = std::move(it->second);
    g_verifiers.erase(it);
    return MZK_OK;
}

extern "C" int32_t mzk_verifier_shape(uint64_t verifier, uint32_t* out_n_proof_points, uint32_t* out_n_key_bases, uint64_t* out_proof_len, uint64_t* out_num_inputs) {
    std::lock_guard<std::mutex> lk(g_vfy_lock);                       // host-only, no device bound: reads under the lock and holds no reference,
    auto it = g_verifiers.find(verifier);                             // so it is never the last holder (mzk_verifier_check likewise)
    if (it == g_verifiers.end()) { set_error("unknown verifier handle"); return MZK_ERR_BAD_HANDLE; }
    const VfyShape& sh = it->second->sh;
    if (out_n_proof_points) *out_n_proof_points = sh.np;
    if (out_n_key_bases) *out_n_key_bases = sh.nkey;
    if (out_proof_len) *out_proof_len = sh.proof_len;
    if (out_num_inputs) *out_num_inputs = sh.num_inputs;
    return MZK_OK;
}

extern "C" int32_t mzk_verifier_batch_begin(uint64_t verifier, const uint8_t* proofs, uint64_t proof_len, uint64_t K, const uint64_t* public_inputs_canonical,
                                            const uint8_t* extra_msgs, const uint64_t* extra_ranges, const uint64_t* challenges_mont, uint32_t flags,
                                            uint64_t* out_batch, uint64_t* out_u_mont, uint64_t* out_bad_index) {
    ON_DEVICE_OF(verifier, v, find_verifier);
    if (v->open_only) { set_error("the verifier holds no verifying key"); return MZK_ERR_INVALID_ARG; }
    if (!proofs || !K || K >= (1ull << 24) || !out_batch || (v->sh.num_inputs && !public_inputs_canonical) || (flags & ~(MZK_SER_VALIDATE | MZK_TRANSCRIPT_SOLIDITY))) {
        set_error("bad argument");
        return MZK_ERR_INVALID_ARG;
    }
    return batch_begin(v, proofs, proof_len, K, public_inputs_canonical, extra_msgs, extra_ranges, challenges_mont, flags, out_batch, out_u_mont, out_bad_index);
}

extern "C" int32_t mzk_batch_proof_layout(int32_t curve_id, uint32_t ultra, uint32_t m, uint32_t flags, const uint8_t* image, uint64_t len,
                                          mzk_batch_proof_layout_t* out) {
    if (!valid_curve(curve_id) || ultra > 1 || !out || !m) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    if (m > MZK_VERIFIER_MAX_INSTANCES) { set_error("more than " + std::to_string(MZK_VERIFIER_MAX_INSTANCES) + " instances in one aggregate"); return MZK_ERR_UNSUPPORTED; }
    batch_proof_layout(g1_bytes(curve_id, flags & MZK_SER_COMPRESSED), ultra, m, *out);
    if (!image) return MZK_OK;
    std::string why;
    uint32_t inst;
    if (batch_proof_container_ok(*out, image, len, inst, why)) return MZK_OK;
    set_error("instance " + std::to_string(inst) + ": " + why);
    return MZK_ERR_ENCODING;
}

extern "C" int32_t mzk_verifier_aggregate_shape(const uint64_t* verifiers, uint32_t m, uint32_t* out_n_proof_points, uint32_t* out_n_key_bases,
                                                uint64_t* out_proof_len, uint64_t* out_num_inputs) {
    MZK_TRY(tuple_args(verifiers, m));
    VfyAggShape ag;
    mzk_batch_proof_layout_t L;
    {
        std::lock_guard<std::mutex> lk(g_vfy_lock);                   // host-only, no device bound: the references (declared after the lock) are dropped
        std::vector<std::shared_ptr<Verifier>> vs;                    // before the lock is, while the registry holds its own: never the last holder
        for (uint32_t j = 0; j < m; j++) {
            auto it = g_verifiers.find(verifiers[j]);
            if (it == g_verifiers.end()) { set_error("unknown verifier handle"); return MZK_ERR_BAD_HANDLE; }
            vs.push_back(it->second);
        }
        MZK_TRY(tuple_shape(vs, ag, L));
    }
    if (out_n_proof_points) *out_n_proof_points = ag.np;
    if (out_n_key_bases) *out_n_key_bases = ag.nkey;
    if (out_proof_len) *out_proof_len = ag.proof_len;
    if (out_num_inputs) *out_num_inputs = ag.total_inputs;
    return MZK_OK;
}

extern "C" int32_t mzk_verifier_aggregate_begin(const uint64_t* verifiers, uint32_t m, const uint8_t* proofs, uint64_t proof_len, uint64_t K,
                                                const uint64_t* public_inputs_canonical, const uint8_t* extra_msgs, const uint64_t* extra_ranges,
                                                const uint64_t* challenges_mont, uint32_t flags, uint64_t* out_batch, uint64_t* out_u_mont,
                                                uint64_t* out_bad_index) {
    MZK_TRY(tuple_args(verifiers, m));
    DeviceGuard guard(handle_ctx(verifiers[0]));                      // the tuple's device (tuple_shape refuses a verifier of another)
    MZK_TRY(guard_status(guard));
    std::vector<std::shared_ptr<Verifier>> vs;                        // declared after the guard: a last reference drops while that device is bound
    MZK_TRY(find_tuple(verifiers, m, vs));
    if (!proofs || !K || K >= (1ull << 24) || !out_batch || (flags & ~(MZK_SER_VALIDATE | MZK_TRANSCRIPT_SOLIDITY))) {
        set_error("bad argument");
        return MZK_ERR_INVALID_ARG;
    }
    return aggregate_begin(vs, proofs, proof_len, K, public_inputs_canonical, extra_msgs, extra_ranges, challenges_mont, flags, out_batch, out_u_mont, out_bad_index);
}

extern "C" int32_t mzk_verifier_batch_challenges(uint64_t batch, uint64_t* out) {
    ON_DEVICE_OF(batch, b, find_batch);
    if (!out) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    if (b->kind == BatchKind::Links) { set_error("a link batch has no challenges: mzk_verifier_link_values"); return MZK_ERR_INVALID_ARG; }
    return hip_status(hipMemcpy(out, b->chal.p, b->K * 7 * 32, hipMemcpyDeviceToHost), "hipMemcpy of the challenges");
}

extern "C" int32_t mzk_verifier_batch_scalars(uint64_t batch, uint64_t* out_key_rows, uint64_t* out_proof_rows, uint64_t* out_evals) {
    ON_DEVICE_OF(batch, b, find_batch);
    if (out_key_rows) HIP_TRY(hipMemcpy(out_key_rows, b->key_rows.p, b->K * b->nkey * 32, hipMemcpyDeviceToHost));
    if (out_proof_rows) HIP_TRY(hipMemcpy(out_proof_rows, b->b_scal.as<uint8_t>() + (size_t)b->nkey * 32, b->K * b->np * 32, hipMemcpyDeviceToHost));
    if (out_evals) HIP_TRY(hipMemcpy(out_evals, b->evals.p, b->K * 32, hipMemcpyDeviceToHost));
    return MZK_OK;
}

extern "C" int32_t mzk_verifier_batch_finish(uint64_t batch, const uint64_t* r_weights_mont, uint64_t* out_A_xyz, uint64_t* out_B_xyz) {
    DeviceGuard guard(handle_ctx(batch));                             // (looked at below: the handle is consumed first, whatever follows)
    const std::shared_ptr<Batch> b = find_batch(batch, true);
    if (!b) return MZK_ERR_BAD_HANDLE;
    MZK_TRY(guard_status(guard));
    if (!r_weights_mont && !out_A_xyz && !out_B_xyz) return MZK_OK;   // discarded
    if (!r_weights_mont || !out_A_xyz || !out_B_xyz) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    return batch_finish(*b, r_weights_mont, out_A_xyz, out_B_xyz);
}

extern "C" int32_t mzk_verifier_check(uint64_t verifier, const uint64_t* A_xyz, const uint64_t* B_xyz, uint64_t n_groups, int32_t* out_accept) {
    int curve = 0;
    std::vector<uint64_t> g2;                                         // (beta_h, h), 2 x 4 L limbs: copied under the lock, no reference held
    {
        std::lock_guard<std::mutex> lk(g_vfy_lock);
        auto it = g_verifiers.find(verifier);
        if (it == g_verifiers.end()) { set_error("unknown verifier handle"); return MZK_ERR_BAD_HANDLE; }
        curve = it->second->curve, g2 = it->second->beta_h;
        g2.insert(g2.end(), it->second->h.begin(), it->second->h.end());
    }
    if (!A_xyz || !B_xyz || !n_groups || !out_accept) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    const size_t L = fq_words(curve) / 2;                             // 64-bit limbs of Fq
    std::vector<uint64_t> sum(2 * 3 * L), g1(2 * 2 * L);
    MZK_TRY(mzk_g1_sum_jacobian(curve, A_xyz, n_groups, &sum[0]));
    MZK_TRY(mzk_g1_sum_jacobian(curve, B_xyz, n_groups, &sum[3 * L]));
    MZK_TRY(mzk_g1_jacobian_to_affine(curve, sum.data(), 2, g1.data()));
    if (curve == MZK_CURVE_BLS12_381) fq_negate_host<BlsFq>(&g1[3 * L]);   // -B
    else fq_negate_host<BnFq>(&g1[3 * L]);
    return mzk_pairing_product_is_one(curve, g1.data(), g2.data(), 2, out_accept);   // e(A, beta_h) e(-B, h) = 1
}

extern "C" int32_t mzk_verifier_create_open_key(int32_t curve_id, const uint8_t* g_bytes, const uint8_t* h_bytes, const uint8_t* beta_h_bytes, uint32_t flags,
                                                uint64_t* out_handle) {
    if (!valid_curve(curve_id) || !g_bytes || !h_bytes || !beta_h_bytes || !out_handle || (flags & ~(MZK_SER_COMPRESSED | MZK_SER_VALIDATE))) {
        set_error("bad argument");
        return MZK_ERR_INVALID_ARG;
    }
    int32_t device;                                                   // the calling thread's context, as mzk_verifier_create
    MZK_TRY(mzk_get_device(&device));
    return open_key_create(curve_id, device, g_bytes, h_bytes, beta_h_bytes, flags, out_handle);
}

extern "C" int32_t mzk_verifier_link_begin(uint64_t verifier, const uint8_t* records, uint64_t K, const uint64_t* layouts, const uint64_t* eta_mont, uint32_t flags,
                                           uint64_t* out_batch, uint64_t* out_eta_mont, uint64_t* out_bad_index) {
    ON_DEVICE_OF(verifier, v, find_verifier);
    if (!records || !K || K >= (1ull << 24) || !layouts || !out_batch || (flags & ~(MZK_SER_VALIDATE | MZK_TRANSCRIPT_SOLIDITY))) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    return link_begin(v, records, K, layouts, eta_mont, flags, out_batch, out_eta_mont, out_bad_index);
}

extern "C" int32_t mzk_verifier_link_values(uint64_t batch, uint64_t* out_eta_mont, uint64_t* out_vanishing_mont) {
    ON_DEVICE_OF(batch, b, find_batch);
    if (b->kind != BatchKind::Links) { set_error("not a link batch"); return MZK_ERR_INVALID_ARG; }
    if (out_eta_mont) HIP_TRY(hipMemcpy(out_eta_mont, b->chal.p, b->K * 32, hipMemcpyDeviceToHost));
    if (out_vanishing_mont) HIP_TRY(hipMemcpy(out_vanishing_mont, b->vanish.p, b->K * 32, hipMemcpyDeviceToHost));
    return MZK_OK;
}

extern "C" int32_t mzk_verifier_link_weights(uint64_t batch, const uint64_t* r_mont, uint64_t* out_weights_mont) {
    ON_DEVICE_OF(batch, b, find_batch);
    if (b->kind != BatchKind::Links) { set_error("not a link batch"); return MZK_ERR_INVALID_ARG; }
    if (!out_weights_mont) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    std::vector<uint64_t> eta(b->K * 4);
    HIP_TRY(hipMemcpy(eta.data(), b->chal.p, b->K * 32, hipMemcpyDeviceToHost));
    if (b->v->curve == MZK_CURVE_BLS12_381) link_weights_t<BlsFr>(r_mont, eta.data(), b->open_recs, b->K, out_weights_mont);
    else link_weights_t<BnFr>(r_mont, eta.data(), b->open_recs, b->K, out_weights_mont);
    return MZK_OK;
}
