// verifier.hip -- mzk_verifier_*: PlonkKzgSnark::batch_verify for single-instance proofs (snark.rs:141-190, verifier.rs:68-251) and
// verify_batch_proof for aggregated BatchProofs under a tuple of keys (snark.rs:117-138; mzk_verifier_aggregate_*), verify_link_proof for
// proof links under an open key (proof_linking.rs:240-286; mzk_verifier_create_open_key, mzk_verifier_link_*), UnivariateKzgPCS::verify /
// batch_verify for KZG openings (univariate_kzg/mod.rs:195-271; mzk_verifier_open_begin).  The per-proof
// work runs on the device (verifier.cuh: decode, Fiat-Shamir, linearisation scalars), the two MSMs through the variable-base path over a base
// array registered per batch, the two pairings on the host (hostpairing.hpp behind mzk_pairing_product_is_one).  A single proof is an
// aggregate of one instance under a tuple of one key: both containers go through proofs_begin, each with the layout of its image.
#include "internal.hpp"
#include "hostfp.hpp"
#include "verifier.cuh"

#include <algorithm>
#include <memory>

namespace mzk {
namespace {

struct Verifier {
    int curve = 0, device = -1;                                   // device: the logical device it was created on, where its memory lives
    VfyAggShape sh{};                                             // a `Proof` image under this key: one instance, total_inputs the key's num_inputs
                                                                  // (sh.compressed: the mode of the key image and of every proof under it)
    DevOwned key_xy, key_inf, k_mont, script;
    DevOwned cols, pos_tab, link_cols, open_cols;                 // the column tables of a `Proof` image, of a link's and of an opening's records, the one-position table (verifier.cuh)
    uint32_t n_items = 0, script_len = 0;
    std::vector<uint64_t> h, beta_h;                              // mzk_g2_decode's output
    std::vector<uint64_t> g;                                      // open_key.g as decoded (host copy: an aggregate's tuple compares open keys)
    bool open_only = false;                                       // mzk_verifier_create_open_key: no verifying key, key_xy holds open_key.g alone
    uint32_t g_index() const { return open_only ? 0 : sh.nkey - 1; }   // open_key.g in key_xy / key_inf
    uint32_t num_inputs() const { return sh.total_inputs; }       // this key's public inputs: the total of a tuple of one
};
enum class BatchKind { Proofs, Links, Openings };                 // Proofs: single proofs and aggregates (two A bases each); Links, Openings: one A base each
struct Batch {
    std::shared_ptr<Verifier> v;                                  // an open batch keeps its verifier alive ...
    std::vector<std::shared_ptr<Verifier>> more;                  // ... and an aggregate batch the verifiers at positions 1 .. m - 1 of its tuple too
    BatchKind kind = BatchKind::Proofs;
    uint64_t K = 0;
    uint32_t np = 0, nkey = 0;                                    // columns of one proof's row and of the key row (an aggregate: NP(m), NKEY(m); links: 4, 1; openings: 2, 1)
    DevOwned images, pub, extra, extra_range, bases, inf, a_bases, a_inf, chal, key_rows, b_scal, evals, a_scal, weights, err;
    DevOwned script, pos_tab, k_mont;                             // a tuple's tables, gathered per position (a tuple of one key reads its verifier's)
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

// the layout of a `Proof` image (structs.rs:59-84) under this key's type and mode: the shape of one instance, its records where the
// stages look for instance 0's (verifier.cuh), the strides unused
void proof_shape(VfyAggShape& sh) {
    const uint32_t W = sh.W, G = sh.g1_bytes;
    sh.m = 1, sh.nkey1 = sh.nsel + W + (sh.ultra ? 4 : 0), sh.nkey = sh.nkey1 + 1, sh.np = 2 * W + 3 + (sh.ultra ? 3 : 0);
    sh.wires_off = 8;                                                            // wires_poly_comms, after its count
    sh.prod_off = sh.wires_off + W * G;                                          // prod_perm_poly_comm
    sh.quot_off = sh.prod_off + G + 8;                                           // split_quot_poly_comms, opening_proof, shifted_opening_proof
    sh.evals_off = sh.quot_off + (W + 2) * G;                                    // wires_evals' count .. perm_next_eval
    sh.plk_off = sh.evals_off + 16 + 32 * 2 * W;                                 // Option<PlookupProof>: tag, count, h (2), prod_lookup, 15 evaluations
    sh.proof_len = sh.plk_off + 1 + (sh.ultra ? 8 + 3 * G + 32 * 15 : 0);
}
std::vector<uint32_t> proof_columns(const VfyAggShape& sh) {      // its G1 records in image order, which is the column order
    const uint32_t W = sh.W, G = sh.g1_bytes;
    std::vector<uint32_t> off;
    for (uint32_t k = 0; k < W + 1; k++) off.push_back(sh.wires_off + k * G);
    for (uint32_t k = 0; k < W + 2; k++) off.push_back(sh.quot_off + k * G);
    for (uint32_t k = 0; k < (sh.ultra ? 3u : 0u); k++) off.push_back(sh.plk_off + 9 + k * G);
    return off;
}
std::string proof_point_name(uint32_t W, uint32_t j) {
    if (j < W) return "wires_poly_comms[" + std::to_string(j) + "]";
    if (j == W) return "prod_perm_poly_comm";
    if (j < 2 * W + 1) return "split_quot_poly_comms[" + std::to_string(j - W - 1) + "]";
    if (j == 2 * W + 1) return "opening_proof";
    if (j == 2 * W + 2) return "shifted_opening_proof";
    if (j < 2 * W + 5) return "plookup_proof.h_poly_comms[" + std::to_string(j - 2 * W - 3) + "]";
    return "plookup_proof.prod_lookup_poly_comm";
}
std::string proof_eval_name(uint32_t W, uint32_t e) {
    static const char* const PLOOKUP[15] = {"range_table_eval", "key_table_eval", "table_dom_sep_eval", "q_dom_sep_eval", "h_1_eval", "q_lookup_eval",
                                            "prod_next_eval", "range_table_next_eval", "key_table_next_eval", "table_dom_sep_next_eval", "h_1_next_eval",
                                            "h_2_next_eval", "q_lookup_next_eval", "w_3_next_eval", "w_4_next_eval"};
    if (e < W) return "wires_evals[" + std::to_string(e) + "]";
    if (e < 2 * W - 1) return "wire_sigma_evals[" + std::to_string(e - W) + "]";
    if (e == 2 * W - 1) return "perm_next_eval";
    return std::string("plookup_proof.") + PLOOKUP[(e - 2 * W) % 15];
}
const char* reason_text(uint32_t reason) { return reason == VFY_REASON_NOT_BELOW_R ? "not below the modulus" : srs_bad_reason((int)reason); }
struct VfyError { uint64_t index; uint32_t inst, field, reason; };   // the stages' error word (vfy_agg_report), taken apart
VfyError error_fields(unsigned long long bad) { return {bad >> 40, (uint32_t)(bad >> 33) & 0x7F, (uint32_t)(bad >> 4) & 0x1FFFFFFF, (uint32_t)bad & 0xF}; }

// Stage A over n_images images `stride` bytes apart.  cols: the np records' offsets, then their field codes, on the device (upload_columns);
// open_idx: the first of the two opening columns, which also go to a_bases -- np where there are none.
template <class X>
void launch_decode(bool compressed, bool validate, const uint8_t* images, uint64_t n_images, uint32_t stride, const uint32_t* cols, uint32_t np, uint32_t open_idx,
                   uint32_t* bases, uint32_t* inf, uint32_t* a_bases, uint32_t* a_inf, unsigned long long* err) {
    const dim3 grid((unsigned)((n_images * np + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
#define MZK_DECODE(C, V)                                                                                                                                \
    hipLaunchKernelGGL((vfy_decode_kernel<X, C, V>), grid, block, 0, nullptr, images, (unsigned long long)n_images, np, stride, cols, cols + np, open_idx, bases, inf, \
                       a_bases, a_inf, err)
    if (compressed) {
        if (validate) MZK_DECODE(true, true);
        else MZK_DECODE(true, false);
    } else {
        if (validate) MZK_DECODE(false, true);
        else MZK_DECODE(false, false);
    }
#undef MZK_DECODE
}
void decode_points(int curve, bool compressed, bool validate, const uint8_t* images, uint64_t n_images, uint32_t stride, const uint32_t* cols, uint32_t np,
                   uint32_t open_idx, uint32_t* bases, uint32_t* inf, uint32_t* a_bases, uint32_t* a_inf, unsigned long long* err) {
    if (curve == MZK_CURVE_BLS12_381) launch_decode<BlsFqX>(compressed, validate, images, n_images, stride, cols, np, open_idx, bases, inf, a_bases, a_inf, err);
    else launch_decode<BnFqX>(compressed, validate, images, n_images, stride, cols, np, open_idx, bases, inf, a_bases, a_inf, err);
}
// a column table on the device: the offsets, then the field codes instance << 8 | field (none given: record j is field j of instance 0)
int32_t upload_columns(DevOwned& cols, std::vector<uint32_t> off, const std::vector<uint32_t>& fld = {}) {
    const uint32_t n = (uint32_t)off.size();
    for (uint32_t j = 0; j < n; j++) off.push_back(fld.empty() ? j : fld[j]);
    MZK_TRY(cols.alloc(off.size() * 4));
    HIP_TRY(hipMemcpy(cols.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    return MZK_OK;
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

// One staged image's G1 records (a verifying key's commitments, an open key's g) decoded into the verifier's key_xy / key_inf, no opening
// columns; bad: the error word, ~0 when every record is sound
int32_t decode_key_image(Verifier& v, bool validate, const uint8_t* image, uint64_t len, const std::vector<uint32_t>& off, unsigned long long& bad) {
    const uint32_t n = (uint32_t)off.size();
    DevOwned staged, cols, err;
    MZK_TRY(staged.alloc(len));
    MZK_TRY(err.alloc(8));
    MZK_TRY(upload_columns(cols, off));
    MZK_TRY(v.key_xy.alloc((size_t)n * 2 * fq_words(v.curve) * 4));
    MZK_TRY(v.key_inf.alloc((size_t)n * 4));
    HIP_TRY(hipMemcpy(staged.p, image, len, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(err.p, 0xFF, 8));
    decode_points(v.curve, v.sh.compressed, validate, staged.as<uint8_t>(), 1, (uint32_t)len, cols.as<uint32_t>(), n, n, v.key_xy.as<uint32_t>(), v.key_inf.as<uint32_t>(),
                  nullptr, nullptr, err.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&bad, err.p, 8, hipMemcpyDeviceToHost));
    return MZK_OK;
}
// h, beta_h: decoded on the host, where the pairing runs; a refusal names them under the caller's prefix
int32_t decode_g2_pair(Verifier& v, uint32_t flags, const uint8_t* h, const uint8_t* beta_h, const char* prefix) {
    const struct { const char* name; const uint8_t* rec; std::vector<uint64_t>& out; } points[2] = {{"h", h, v.h}, {"beta_h", beta_h, v.beta_h}};
    for (const auto& pt : points) {
        pt.out.resize(4 * fq_words(v.curve) / 2);
        if (mzk_g2_decode(v.curve, pt.rec, flags & (MZK_SER_COMPRESSED | MZK_SER_VALIDATE), pt.out.data()) != MZK_OK) {
            set_error(std::string(prefix) + pt.name + ": " + mzk_last_error());
            return MZK_ERR_ENCODING;
        }
    }
    return MZK_OK;
}
// A link's four records stand back to back, an opening's two: their column tables, kept on every verifier (either kind verifies links
// and openings) so that link_begin and open_begin upload nothing
int32_t upload_link_columns(Verifier& v) {
    const uint32_t G = v.sh.g1_bytes;
    MZK_TRY(upload_columns(v.open_cols, {0, G}));
    return upload_columns(v.link_cols, {0, G, 2 * G, 3 * G});
}
int32_t publish_verifier(std::shared_ptr<Verifier> v, uint64_t* out_handle) {
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    *out_handle = handle_make(v->device, g_next_verifier++);
    g_verifiers[*out_handle] = std::move(v);
    return MZK_OK;
}

int32_t verifier_create(int32_t curve, int device, const uint8_t* vk, uint64_t len, uint32_t flags, uint64_t* out_handle) {
    const bool compressed = flags & MZK_SER_COMPRESSED;
    mzk_key_layout_t lay;
    MZK_TRY(mzk_key_layout(curve, vk, len, (flags & MZK_SER_COMPRESSED) | MZK_KEY_VK_ONLY, &lay));
    if (lay.is_merged) { set_error("merged verifying keys are not supported"); return MZK_ERR_UNSUPPORTED; }
    if (len >= (1ull << 31)) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    auto v = std::make_shared<Verifier>();
    v->curve = curve, v->device = device;
    VfyAggShape& sh = v->sh;
    sh.W = lay.num_wire_types, sh.nsel = lay.num_selectors, sh.ultra = lay.has_plookup_vk, sh.n = lay.domain_size, sh.total_inputs = (uint32_t)lay.num_inputs;
    if (lay.num_inputs > lay.domain_size) { set_error("num_inputs: larger than the domain"); return MZK_ERR_ENCODING; }
    for (sh.log_n = 0; (1ull << sh.log_n) < sh.n; sh.log_n++) {}
    sh.compressed = compressed, sh.g1_bytes = g1_bytes(curve, compressed);
    proof_shape(sh);
    const uint32_t G = sh.g1_bytes, nkey = sh.nkey, fqw = fq_words(curve);
    // the key's commitments, decoded on the device; infinity is a normal value here (an unused selector commits to nothing)
    std::vector<uint32_t> off;
    std::vector<std::string> names;
    for (uint32_t j = 0; j < sh.nsel; j++) { off.push_back((uint32_t)(lay.selector_comms_off + j * G)); names.push_back("selector_comms[" + std::to_string(j) + "]"); }
    for (uint32_t j = 0; j < sh.W; j++) { off.push_back((uint32_t)(lay.sigma_comms_off + j * G)); names.push_back("sigma_comms[" + std::to_string(j) + "]"); }
    static const char* const PLK[4] = {"range_table_comm", "key_table_comm", "table_dom_sep_comm", "q_dom_sep_comm"};
    if (sh.ultra)
        for (uint32_t j = 0; j < 4; j++) { off.push_back((uint32_t)(lay.plookup_comms_off + j * G)); names.push_back(std::string("plookup_vk.") + PLK[j]); }
    off.push_back((uint32_t)lay.g_off);
    names.push_back("open_key.g");
    unsigned long long bad = 0;
    MZK_TRY(decode_key_image(*v, flags & MZK_SER_VALIDATE, vk, len, off, bad));
    if (bad != ~0ull) {
        const VfyError e = error_fields(bad);
        set_error("vk." + names[e.field] + ": " + reason_text(e.reason));
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
    // what stages A to C read of a tuple, for the tuple of this key alone: a `Proof` image's columns, one position's { script, items, inputs }
    const uint32_t pos_tab[6] = {0, v->n_items, 0, v->script_len, 0, v->num_inputs()};
    MZK_TRY(upload_columns(v->cols, proof_columns(sh)));
    MZK_TRY(v->pos_tab.alloc(sizeof pos_tab));
    HIP_TRY(hipMemcpy(v->pos_tab.p, pos_tab, sizeof pos_tab, hipMemcpyHostToDevice));
    MZK_TRY(decode_g2_pair(*v, flags, vk + lay.h_off, vk + lay.beta_h_off, "vk.open_key."));
    MZK_TRY(upload_link_columns(*v));
    return publish_verifier(std::move(v), out_handle);
}

// the container of proof i on the host: Vec counts and the Option tag against the key's type
bool proof_container_ok(const VfyAggShape& sh, const uint8_t* img, std::string& why) {
    const auto count = [&](uint32_t off) { uint64_t c; std::memcpy(&c, img + off, 8); return c; };
    const auto expect = [&](const char* field, uint32_t off, uint64_t want) {
        if (count(off) == want) return true;
        why = std::string(field) + ".len: " + std::to_string(count(off)) + ", expected " + std::to_string(want);
        return false;
    };
    const uint32_t W = sh.W;
    if (!expect("wires_poly_comms", 0, W) || !expect("split_quot_poly_comms", sh.quot_off - 8, W) || !expect("wires_evals", sh.evals_off, W) ||
        !expect("wire_sigma_evals", sh.evals_off + 8 + 32 * W, W - 1))
        return false;
    const uint8_t tag = img[sh.plk_off];
    if (tag != (sh.ultra ? 1 : 0)) {
        why = tag > 1 ? "plookup_proof: invalid Option tag" : sh.ultra ? "plookup_proof: absent under an UltraPlonk key" : "plookup_proof: present under a TurboPlonk key";
        return false;
    }
    return !sh.ultra || expect("plookup_proof.h_poly_comms", sh.plk_off + 1, 2);
}

// Stage B under MZK_TRANSCRIPT_SOLIDITY keeps each transcript in a slot of device memory (verifier.cuh, vfy_transcript_init): the 64 bytes of
// the state, at most `transcript_bytes` of transcript and the recorded challenge points, for every thread of the ceil(K / 64) blocks.
int32_t alloc_slots(DevOwned& slots, uint64_t K, uint64_t transcript_bytes, uint32_t& slot_words) {
    slot_words = keccak::SolidityTranscript::slot_words(transcript_bytes);
    return slots.alloc((K + VFY_THREADS - 1) / VFY_THREADS * VFY_THREADS * slot_words * 8);
}
// the curve and the transcript kind of a stage B launch: f(StageB<Fr, FqX, T>{})
template <class A, class B, class C>
struct StageB { using Fr = A; using FqX = B; using T = C; };
template <class F>
void with_transcript(int curve, bool solidity, F&& f) {
    if (curve == MZK_CURVE_BLS12_381) solidity ? f(StageB<BlsFr, BlsFqX, keccak::SolidityTranscript>{}) : f(StageB<BlsFr, BlsFqX, merlin::Transcript>{});
    else solidity ? f(StageB<BnFr, BnFqX, keccak::SolidityTranscript>{}) : f(StageB<BnFr, BnFqX, merlin::Transcript>{});
}
// the proofs' extra messages: `end` of the blob their ranges need, and the longest message
int32_t check_extra(const uint8_t* extra, const uint64_t* extra_ranges, uint64_t K, uint64_t& end, uint64_t& longest) {
    end = longest = 0;
    if (extra_ranges)
        for (uint64_t i = 0; i < K; i++) {
            const uint64_t b = extra_ranges[2 * i], e = extra_ranges[2 * i + 1];
            if (b == ~0ull) continue;
            if (e < b || e - b >= (1ull << 31) || !extra) { set_error("bad extra message range"); return MZK_ERR_INVALID_ARG; }
            end = std::max(end, e), longest = std::max(longest, e - b);
        }
    return MZK_OK;
}
// What every batch has: its K images staged in one copy, the base and scalar arrays of its np + nkey columns, n_chal values of 32 bytes
// in chal and n_a bases of the MSM A per member, the error word set.  (b.v, b.K, b.np and b.nkey are the caller's.)
int32_t stage_batch(Batch& b, const uint8_t* images, uint64_t image_len, uint32_t n_chal, uint32_t n_a) {
    const uint64_t K = b.K;
    const size_t pt_bytes = (size_t)2 * fq_words(b.v->curve) * 4, n_bases = b.nkey + K * b.np;
    MZK_TRY(b.images.alloc(K * image_len));
    MZK_TRY(b.bases.alloc(n_bases * pt_bytes));
    MZK_TRY(b.inf.alloc(n_bases * 4));
    MZK_TRY(b.a_bases.alloc(n_a * K * pt_bytes));
    MZK_TRY(b.a_inf.alloc(n_a * K * 4));
    MZK_TRY(b.chal.alloc(K * n_chal * 32));
    MZK_TRY(b.key_rows.alloc(K * b.nkey * 32));
    MZK_TRY(b.b_scal.alloc(n_bases * 32));
    MZK_TRY(b.evals.alloc(K * 32));
    MZK_TRY(b.a_scal.alloc(n_a * K * 32));
    MZK_TRY(b.weights.alloc(K * 32));
    MZK_TRY(b.err.alloc(8));
    HIP_TRY(hipMemcpy(b.images.p, images, K * image_len, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b.err.p, 0xFF, 8));
    return MZK_OK;
}
// The end of every begin: the error word, whose copy synchronises the stages -- `<member> <i>: <name(instance, field)>: <reason>` for the
// lowest bad member -- else the batch hands out one value of chal per member (32 bytes at `first`, every `pitch` bytes) and is
// published under the lock, last.
template <class Name>
int32_t publish_batch(std::shared_ptr<Batch> b, const char* member, Name name, uint64_t* out_values, size_t first, size_t pitch, uint64_t* out_batch, uint64_t* out_bad) {
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpy(&bad, b->err.p, 8, hipMemcpyDeviceToHost));
    if (bad != ~0ull) {
        const VfyError e = error_fields(bad);
        if (out_bad) *out_bad = e.index;
        set_error(std::string(member) + " " + std::to_string(e.index) + ": " + name(e.inst, e.field) + ": " + reason_text(e.reason));
        return MZK_ERR_ENCODING;
    }
    if (out_values) HIP_TRY(hipMemcpy2D(out_values, 32, b->chal.as<uint8_t>() + first, pitch, 32, b->K, hipMemcpyDeviceToHost));
    std::lock_guard<std::mutex> lk(g_vfy_lock);
    *out_batch = handle_make(b->v->device, g_next_batch++);
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
    const bool links = b.kind != BatchKind::Proofs;                   // a link, an opening: A over its one opening proof
    if (v.curve == MZK_CURVE_BLS12_381) links ? launch_finish<BlsFr, 1>(b, K, np, nkey) : launch_finish<BlsFr, 2>(b, K, np, nkey);
    else links ? launch_finish<BnFr, 1>(b, K, np, nkey) : launch_finish<BnFr, 2>(b, K, np, nkey);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    // the two MSMs of verifier.rs:217-247 through the variable-base path (links, openings: A over the K opening proofs)
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
        total_inputs += v.num_inputs();
    }
    if (total_inputs >= (1ull << 28)) { set_error("too many public inputs"); return MZK_ERR_UNSUPPORTED; }
    const VfyAggShape& s = v0.sh;
    batch_proof_layout(s.g1_bytes, s.ultra, m, L);
    ag = s;                                                                          // the type, the mode and the domain; then what m instances change
    ag.m = m, ag.nkey = m * s.nkey1 + 1;
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
    if (field >= VFY_FIELD_PUB_INPUT) return "public_input[" + std::to_string(field - VFY_FIELD_PUB_INPUT) + "]";
    if (field >= VFY_FIELD_EVAL) return proof_eval_name(W, field - VFY_FIELD_EVAL);
    if (inst == ag.m) return field < W ? "split_quot_poly_comms[" + std::to_string(field) + "]" : field == W ? "opening_proof" : "shifted_opening_proof";
    if (field < W) return "wires_poly_comms[" + std::to_string(field) + "]";
    if (field == W) return "prod_perm_poly_comm";
    return field < W + 3 ? "plookup_proof.h_poly_comms[" + std::to_string(field - W - 1) + "]" : "plookup_proof.prod_lookup_poly_comm";
}

template <class Fr>
void launch_agg_scalars(const Batch& b, uint64_t K, const VfyAggShape& ag, const uint32_t* k_mont, const uint32_t* pos_tab, uint32_t* proof_rows, unsigned long long* err) {
    const dim3 grid((unsigned)((K * ag.m + VFY_THREADS - 1) / VFY_THREADS)), fold((unsigned)((K + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
    uint32_t* partials = b.chal.as<uint32_t>() + K * 7 * 8;           // K x m, behind the K x 7 challenges (proofs_begin)
    if (ag.ultra)
        hipLaunchKernelGGL((vfy_agg_scalars_kernel<Fr, true>), grid, block, 0, nullptr, b.images.as<uint8_t>(), (unsigned long long)K, ag, k_mont, pos_tab,
                           b.pub.as<uint32_t>(), b.chal.as<uint32_t>(), b.key_rows.as<uint32_t>(), proof_rows, partials, err);
    else
        hipLaunchKernelGGL((vfy_agg_scalars_kernel<Fr, false>), grid, block, 0, nullptr, b.images.as<uint8_t>(), (unsigned long long)K, ag, k_mont, pos_tab,
                           b.pub.as<uint32_t>(), b.chal.as<uint32_t>(), b.key_rows.as<uint32_t>(), proof_rows, partials, err);
    hipLaunchKernelGGL((vfy_agg_fold_kernel<Fr>), fold, block, 0, nullptr, (unsigned long long)K, ag, b.chal.as<uint32_t>(), partials,
                       b.key_rows.as<uint32_t>(), proof_rows, b.evals.as<uint32_t>());
}

// Stages A, B and C over K images under the tuple vs.  ag and cols (on the device) describe the image: a `Proof` under its verifier's own
// table, whose refusals read `proof i: <field>`, or a BatchProof (batch_proofs), `proof i: instance j: <field>`.  A tuple of one key reads
// that verifier's script, k and position table where they are -- the batch keeps its verifiers alive -- and its key block is the head of
// the base array as it stands; a longer tuple gathers them per POSITION: a repeated key repeats its block, its script and its k.
int32_t proofs_begin(const std::vector<std::shared_ptr<Verifier>>& vs, const VfyAggShape& ag, const uint32_t* cols, bool batch_proofs, const uint8_t* proofs,
                     uint64_t K, const uint64_t* pub, const uint8_t* extra, const uint64_t* extra_ranges, const uint64_t* challenges, uint32_t flags,
                     uint64_t* out_batch, uint64_t* out_u, uint64_t* out_bad) {
    const Verifier& v0 = *vs[0];
    const uint32_t m = ag.m, W = ag.W, np = ag.np, nkey = ag.nkey, nkey1 = ag.nkey1;
    uint64_t extra_len, longest_extra;
    MZK_TRY(check_extra(extra, extra_ranges, K, extra_len, longest_extra));
    const int curve = v0.curve;
    const uint32_t fqw = fq_words(curve);
    const size_t pt_bytes = (size_t)2 * fqw * 4;
    auto b = std::make_shared<Batch>();                               // (a failure below frees it here, under the caller's guard)
    b->v = vs[0], b->more.assign(vs.begin() + 1, vs.end()), b->K = K, b->np = np, b->nkey = nkey;
    MZK_TRY(stage_batch(*b, proofs, ag.proof_len, 7 + m, 2));        // chal: the K x 7 challenges, then stage C's K x m partial evaluations
    MZK_TRY(b->pub.alloc(K * ag.total_inputs * 32));
    MZK_TRY(b->extra.alloc(extra_len));
    MZK_TRY(b->extra_range.alloc(K * 16));
    if (ag.total_inputs) HIP_TRY(hipMemcpy(b->pub.p, pub, K * ag.total_inputs * 32, hipMemcpyHostToDevice));
    if (extra_len) HIP_TRY(hipMemcpy(b->extra.p, extra, extra_len, hipMemcpyHostToDevice));
    if (extra_ranges) HIP_TRY(hipMemcpy(b->extra_range.p, extra_ranges, K * 16, hipMemcpyHostToDevice));
    const uint8_t* script = v0.script.as<uint8_t>();
    const uint32_t *pos_tab = v0.pos_tab.as<uint32_t>(), *k_mont = v0.k_mont.as<uint32_t>();
    uint32_t script_len = v0.script_len;
    if (m == 1) {
        HIP_TRY(hipMemcpyAsync(b->bases.p, v0.key_xy.p, nkey * pt_bytes, hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(b->inf.p, v0.key_inf.p, nkey * 4, hipMemcpyDeviceToDevice, nullptr));
    } else {
        std::vector<uint32_t> tab;
        uint32_t inputs = 0;
        script_len = 0;
        for (uint32_t j = 0; j < m; j++) {
            tab.insert(tab.end(), {script_len, vs[j]->n_items, inputs});
            script_len += vs[j]->script_len, inputs += vs[j]->num_inputs();
        }
        tab.insert(tab.end(), {script_len, 0u, inputs});
        MZK_TRY(b->script.alloc(script_len));
        MZK_TRY(b->pos_tab.alloc(tab.size() * 4));
        MZK_TRY(b->k_mont.alloc((size_t)m * W * 32));
        HIP_TRY(hipMemcpy(b->pos_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        for (uint32_t j = 0; j < m; j++) {
            const Verifier& v = *vs[j];
            HIP_TRY(hipMemcpyAsync(b->bases.as<uint8_t>() + (size_t)j * nkey1 * pt_bytes, v.key_xy.p, nkey1 * pt_bytes, hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(b->inf.as<uint32_t>() + (size_t)j * nkey1, v.key_inf.p, nkey1 * 4, hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(b->script.as<uint8_t>() + tab[3 * j], v.script.p, v.script_len, hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(b->k_mont.as<uint8_t>() + (size_t)j * W * 32, v.k_mont.p, (size_t)W * 32, hipMemcpyDeviceToDevice, nullptr));
        }
        HIP_TRY(hipMemcpyAsync(b->bases.as<uint8_t>() + (size_t)(nkey - 1) * pt_bytes, v0.key_xy.as<uint8_t>() + (size_t)nkey1 * pt_bytes, pt_bytes, hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(b->inf.as<uint32_t>() + (nkey - 1), v0.key_inf.as<uint32_t>() + nkey1, 4, hipMemcpyDeviceToDevice, nullptr));
        script = b->script.as<uint8_t>(), pos_tab = b->pos_tab.as<uint32_t>(), k_mont = b->k_mont.as<uint32_t>();
    }
    unsigned long long* err = b->err.as<unsigned long long>();
    uint32_t* proof_rows = b->b_scal.as<uint32_t>() + (size_t)nkey * 8;
    // A
    decode_points(curve, ag.compressed, flags & MZK_SER_VALIDATE, b->images.as<uint8_t>(), K, ag.proof_len, cols, np, m * (W + 1) + W,
                  b->bases.as<uint32_t>() + (size_t)nkey * 2 * fqw, b->inf.as<uint32_t>() + nkey, b->a_bases.as<uint32_t>(), b->a_inf.as<uint32_t>(), err);
    HIP_TRY(hipGetLastError());
    // B, or the caller's challenges
    DevOwned slots;                                                   // Solidity: the transcripts' memory, freed when the stages are through
    if (challenges) {
        HIP_TRY(hipMemcpy(b->chal.p, challenges, K * 7 * 32, hipMemcpyHostToDevice));
    } else {
        ProfScope ps("vfy_transcript", nullptr, v0.device);
        const dim3 grid((unsigned)((K + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
        const unsigned long long* ranges = extra_ranges ? b->extra_range.as<unsigned long long>() : nullptr;
        const bool solidity = flags & MZK_TRANSCRIPT_SOLIDITY;
        uint32_t slot_words = 0;
        // (the scripts' length bounds their messages; the proof's own: np commitments in compressed form, 2 W (+ 6) evaluations an instance)
        if (solidity)
            MZK_TRY(alloc_slots(slots, K, longest_extra + script_len + 32ull * ag.total_inputs + (uint64_t)np * g1_bytes(curve, true) + 32ull * m * (2 * W + 6),
                                slot_words));
        with_transcript(curve, solidity, [&](auto k) {
            using S = decltype(k);
            hipLaunchKernelGGL((vfy_agg_transcript_kernel<typename S::Fr, typename S::FqX, typename S::T>), grid, block, 0, nullptr, b->images.as<uint8_t>(),
                               (unsigned long long)K, ag, script, pos_tab, b->pub.as<uint32_t>(), b->extra.as<uint8_t>(), ranges, b->chal.as<uint32_t>(),
                               slots.as<uint64_t>(), slot_words);
        });
        HIP_TRY(hipGetLastError());
    }
    // C and the fold
    if (curve == MZK_CURVE_BLS12_381) launch_agg_scalars<BlsFr>(*b, K, ag, k_mont, pos_tab, proof_rows, err);
    else launch_agg_scalars<BnFr>(*b, K, ag, k_mont, pos_tab, proof_rows, err);
    HIP_TRY(hipGetLastError());
    const auto name = [&](uint32_t inst, uint32_t field) {
        if (batch_proofs) return "instance " + std::to_string(inst) + ": " + agg_field_name(ag, inst, field);
        return field < VFY_FIELD_EVAL ? proof_point_name(W, field) : agg_field_name(ag, inst, field);
    };
    return publish_batch(std::move(b), "proof", name, out_u, 6 * 32, 7 * 32, out_batch, out_bad);
}

int32_t batch_begin(const std::shared_ptr<Verifier>& vp, const uint8_t* proofs, uint64_t proof_len, uint64_t K, const uint64_t* pub, const uint8_t* extra,
                    const uint64_t* extra_ranges, const uint64_t* challenges, uint32_t flags, uint64_t* out_batch, uint64_t* out_u, uint64_t* out_bad) {
    const VfyAggShape& sh = vp->sh;
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
    return proofs_begin({vp}, sh, vp->cols.as<uint32_t>(), false, proofs, K, pub, extra, extra_ranges, challenges, flags, out_batch, out_u, out_bad);
}

int32_t aggregate_begin(const std::vector<std::shared_ptr<Verifier>>& vs, const uint8_t* proofs, uint64_t proof_len, uint64_t K, const uint64_t* pub,
                        const uint8_t* extra, const uint64_t* extra_ranges, const uint64_t* challenges, uint32_t flags, uint64_t* out_batch, uint64_t* out_u,
                        uint64_t* out_bad) {
    VfyAggShape ag;
    mzk_batch_proof_layout_t L;
    MZK_TRY(tuple_shape(vs, ag, L));
    if (ag.total_inputs && !pub) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    const uint32_t m = ag.m, W = ag.W, G = ag.g1_bytes;
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
    // the columns of stage A (offset; instance << 8 | field): what belongs to the whole proof counts as instance m
    std::vector<uint32_t> col_off, col_fld;
    const auto col = [&](uint64_t off, uint32_t inst, uint32_t field) { col_off.push_back((uint32_t)off); col_fld.push_back(inst << 8 | field); };
    for (uint32_t j = 0; j < m; j++) {
        for (uint32_t k = 0; k < W; k++) col(L.wires_off[j] + (uint64_t)k * G, j, k);
        col(L.prod_perm_off[j], j, W);
    }
    for (uint32_t k = 0; k < W; k++) col(L.split_quot_off + (uint64_t)k * G, m, k);
    col(L.opening_off, m, W);
    col(L.shifted_opening_off, m, W + 1);
    if (ag.ultra)
        for (uint32_t j = 0; j < m; j++) {
            col(L.h_off[j], j, W + 1);
            col(L.h_off[j] + G, j, W + 2);
            col(L.prod_lookup_off[j], j, W + 3);
        }
    DevOwned cols;                                                    // (the stages are through when proofs_begin returns)
    MZK_TRY(upload_columns(cols, col_off, col_fld));
    return proofs_begin(vs, ag, cols.as<uint32_t>(), true, proofs, K, pub, extra, extra_ranges, challenges, flags, out_batch, out_u, out_bad);
}

// ---- proof links (proof_linking.rs:240-286; verifier.cuh "proof links") ---------------------------------------------------------------------
int32_t open_key_create(int32_t curve, int device, const uint8_t* g_bytes, const uint8_t* h_bytes, const uint8_t* beta_h_bytes, uint32_t flags, uint64_t* out_handle) {
    const bool compressed = flags & MZK_SER_COMPRESSED;
    auto v = std::make_shared<Verifier>();
    v->curve = curve, v->device = device, v->open_only = true;
    v->sh.compressed = compressed, v->sh.g1_bytes = g1_bytes(curve, compressed);       // np = nkey = proof_len = 0: no verifying key
    const uint32_t fqw = fq_words(curve);
    unsigned long long bad = 0;
    MZK_TRY(decode_key_image(*v, flags & MZK_SER_VALIDATE, g_bytes, v->sh.g1_bytes, {0u}, bad));
    if (bad != ~0ull) {
        set_error(std::string("open_key.g: ") + reason_text(error_fields(bad).reason));
        return MZK_ERR_ENCODING;
    }
    uint32_t inf = 0;
    v->g.resize((size_t)2 * fqw / 2);
    HIP_TRY(hipMemcpy(v->g.data(), v->key_xy.p, (size_t)2 * fqw * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&inf, v->key_inf.p, 4, hipMemcpyDeviceToHost));
    if (inf) std::fill(v->g.begin(), v->g.end(), 0);                 // (0, 0): as verifier_create keeps a flagged g
    MZK_TRY(decode_g2_pair(*v, flags, h_bytes, beta_h_bytes, "open_key."));
    MZK_TRY(upload_link_columns(*v));
    return publish_verifier(std::move(v), out_handle);
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
    const size_t pt_bytes = (size_t)2 * fqw * 4;
    auto b = std::make_shared<Batch>();                               // (a failure below frees it here, under the caller's guard)
    b->v = vp, b->kind = BatchKind::Links, b->K = K, b->np = np, b->nkey = nkey;
    b->open_recs.resize(K * G);
    for (uint64_t i = 0; i < K; i++) std::memcpy(&b->open_recs[i * G], records + (i * 4 + 3) * G, G);
    MZK_TRY(stage_batch(*b, records, 4 * G, 1, 1));
    MZK_TRY(b->layouts.alloc(K * 24));
    MZK_TRY(b->vanish.alloc(K * 32));
    HIP_TRY(hipMemcpy(b->layouts.p, layouts, K * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b->key_rows.p, 0, K * nkey * 32));              // open_key.g: scalar zero, and the opened value is 0
    HIP_TRY(hipMemset(b->evals.p, 0, K * 32));
    HIP_TRY(hipMemcpy(b->bases.p, v.key_xy.as<uint8_t>() + (size_t)v.g_index() * pt_bytes, pt_bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(b->inf.p, v.key_inf.as<uint32_t>() + v.g_index(), 4, hipMemcpyDeviceToDevice));
    unsigned long long* err = b->err.as<unsigned long long>();
    // A: no opening columns; the opening proofs (column 3) are then gathered as the bases of the MSM A
    uint8_t* own_bases = b->bases.as<uint8_t>() + (size_t)nkey * pt_bytes;
    decode_points(curve, v.sh.compressed, flags & MZK_SER_VALIDATE, b->images.as<uint8_t>(), K, 4 * G, v.link_cols.as<uint32_t>(), np, np, reinterpret_cast<uint32_t*>(own_bases),
                  b->inf.as<uint32_t>() + nkey, nullptr, nullptr, err);
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
        with_transcript(curve, solidity, [&](auto k) {
            using S = decltype(k);
            hipLaunchKernelGGL((vfy_link_transcript_kernel<typename S::Fr, typename S::FqX, typename S::T>), grid, block, 0, nullptr, b->images.as<uint8_t>(),
                               (unsigned long long)K, G, v.sh.compressed, b->chal.as<uint32_t>(), slots.as<uint64_t>(), slot_words);
        });
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
    return publish_batch(std::move(b), "link", [](uint32_t, uint32_t field) { return std::string(LINK_FIELDS[field & 3]); }, out_eta, 0, 32, out_batch, out_bad);
}

// ---- KZG openings (univariate_kzg/mod.rs:195-271; verifier.cuh "KZG openings") ----------------------------------------------------------------
const char* const OPEN_FIELDS[4] = {"commitment", "proof", "point", "value"};
const char* kind_name(BatchKind k) { return k == BatchKind::Links ? "a link batch" : k == BatchKind::Openings ? "an openings batch" : "a proof batch"; }

int32_t open_begin(const std::shared_ptr<Verifier>& vp, const uint8_t* records, uint64_t K, const uint64_t* points, const uint64_t* values, uint32_t flags,
                   uint64_t* out_batch, uint64_t* out_bad) {
    const Verifier& v = *vp;
    const int curve = v.curve;
    if (out_bad) *out_bad = ~0ull;
    const uint32_t G = v.sh.g1_bytes, np = 2, nkey = 1, fqw = fq_words(curve);
    const size_t pt_bytes = (size_t)2 * fqw * 4;
    auto b = std::make_shared<Batch>();                               // (a failure below frees it here, under the caller's guard)
    b->v = vp, b->kind = BatchKind::Openings, b->K = K, b->np = np, b->nkey = nkey;
    MZK_TRY(stage_batch(*b, records, 2 * G, 1, 1));                   // chal: z_i in Montgomery form
    MZK_TRY(b->pub.alloc(K * 64));                                    // the K points, then the K values, as they came
    HIP_TRY(hipMemcpy(b->pub.p, points, K * 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->pub.as<uint8_t>() + K * 32, values, K * 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->bases.p, v.key_xy.as<uint8_t>() + (size_t)v.g_index() * pt_bytes, pt_bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(b->inf.p, v.key_inf.as<uint32_t>() + v.g_index(), 4, hipMemcpyDeviceToDevice));
    unsigned long long* err = b->err.as<unsigned long long>();
    // A: no opening columns; the opening proofs (column 1) are then gathered as the bases of the MSM A
    uint8_t* own_bases = b->bases.as<uint8_t>() + (size_t)nkey * pt_bytes;
    decode_points(curve, v.sh.compressed, flags & MZK_SER_VALIDATE, b->images.as<uint8_t>(), K, 2 * G, v.open_cols.as<uint32_t>(), np, np, reinterpret_cast<uint32_t*>(own_bases),
                  b->inf.as<uint32_t>() + nkey, nullptr, nullptr, err);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(b->a_bases.p, pt_bytes, own_bases + pt_bytes, 2 * pt_bytes, pt_bytes, K, hipMemcpyDeviceToDevice, nullptr));
    // Co
    {
        ProfScope ps("vfy_open_rows", nullptr, v.device);
        uint32_t* proof_rows = b->b_scal.as<uint32_t>() + (size_t)nkey * 8;
        const uint32_t *pts = b->pub.as<uint32_t>(), *vals = pts + K * 8;
        const dim3 grid((unsigned)((K + VFY_THREADS - 1) / VFY_THREADS)), block(VFY_THREADS);
        if (curve == MZK_CURVE_BLS12_381)
            hipLaunchKernelGGL((vfy_open_rows_kernel<BlsFr>), grid, block, 0, nullptr, (unsigned long long)K, pts, vals, b->inf.as<uint32_t>() + nkey, b->a_inf.as<uint32_t>(),
                               b->chal.as<uint32_t>(), b->key_rows.as<uint32_t>(), proof_rows, b->evals.as<uint32_t>(), err);
        else
            hipLaunchKernelGGL((vfy_open_rows_kernel<BnFr>), grid, block, 0, nullptr, (unsigned long long)K, pts, vals, b->inf.as<uint32_t>() + nkey, b->a_inf.as<uint32_t>(),
                               b->chal.as<uint32_t>(), b->key_rows.as<uint32_t>(), proof_rows, b->evals.as<uint32_t>(), err);
        HIP_TRY(hipGetLastError());
    }
    return publish_batch(std::move(b), "opening", [](uint32_t, uint32_t field) { return std::string(OPEN_FIELDS[field & 3]); }, nullptr, 0, 32, out_batch, out_bad);
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
    const VfyAggShape& sh = it->second->sh;
    if (out_n_proof_points) *out_n_proof_points = sh.np;
    if (out_n_key_bases) *out_n_key_bases = sh.nkey;
    if (out_proof_len) *out_proof_len = sh.proof_len;
    if (out_num_inputs) *out_num_inputs = it->second->num_inputs();
    return MZK_OK;
}

extern "C" int32_t mzk_verifier_batch_begin(uint64_t verifier, const uint8_t* proofs, uint64_t proof_len, uint64_t K, const uint64_t* public_inputs_canonical,
                                            const uint8_t* extra_msgs, const uint64_t* extra_ranges, const uint64_t* challenges_mont, uint32_t flags,
                                            uint64_t* out_batch, uint64_t* out_u_mont, uint64_t* out_bad_index) {
    ON_DEVICE_OF(verifier, v, find_verifier);
    if (v->open_only) { set_error("the verifier holds no verifying key"); return MZK_ERR_INVALID_ARG; }
    if (!proofs || !K || K >= (1ull << 24) || !out_batch || (v->num_inputs() && !public_inputs_canonical) || (flags & ~(MZK_SER_VALIDATE | MZK_TRANSCRIPT_SOLIDITY))) {
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
    if (b->kind == BatchKind::Openings) { set_error("an openings batch has no challenges"); return MZK_ERR_INVALID_ARG; }
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
    if (b->kind != BatchKind::Links) { set_error(std::string("not a link batch: ") + kind_name(b->kind)); return MZK_ERR_INVALID_ARG; }
    if (out_eta_mont) HIP_TRY(hipMemcpy(out_eta_mont, b->chal.p, b->K * 32, hipMemcpyDeviceToHost));
    if (out_vanishing_mont) HIP_TRY(hipMemcpy(out_vanishing_mont, b->vanish.p, b->K * 32, hipMemcpyDeviceToHost));
    return MZK_OK;
}

extern "C" int32_t mzk_verifier_link_weights(uint64_t batch, const uint64_t* r_mont, uint64_t* out_weights_mont) {
    ON_DEVICE_OF(batch, b, find_batch);
    if (b->kind != BatchKind::Links) { set_error(std::string("not a link batch: ") + kind_name(b->kind)); return MZK_ERR_INVALID_ARG; }
    if (!out_weights_mont) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    std::vector<uint64_t> eta(b->K * 4);
    HIP_TRY(hipMemcpy(eta.data(), b->chal.p, b->K * 32, hipMemcpyDeviceToHost));
    if (b->v->curve == MZK_CURVE_BLS12_381) link_weights_t<BlsFr>(r_mont, eta.data(), b->open_recs, b->K, out_weights_mont);
    else link_weights_t<BnFr>(r_mont, eta.data(), b->open_recs, b->K, out_weights_mont);
    return MZK_OK;
}

extern "C" int32_t mzk_verifier_open_begin(uint64_t verifier, const uint8_t* records, uint64_t K, const uint64_t* points_canonical, const uint64_t* values_canonical,
                                           uint32_t flags, uint64_t* out_batch, uint64_t* out_bad_index) {
    ON_DEVICE_OF(verifier, v, find_verifier);
    if (!records || !K || K >= (1ull << 24) || !points_canonical || !values_canonical || !out_batch || (flags & ~MZK_SER_VALIDATE)) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    return open_begin(v, records, K, points_canonical, values_canonical, flags, out_batch, out_bad_index);
}
