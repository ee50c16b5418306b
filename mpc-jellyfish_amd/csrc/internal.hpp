// internal.hpp -- state and helpers shared by the translation units of libmi355zk.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mzk.h"

// library-internal entry point (not in include/mzk.h, not exported): the calling thread's context hands a prover handle its stream
extern "C" int32_t mzk_ctx_prover_stream(uint32_t k, void** out_stream);
// ... and runs the witness check of a prover handle on its proving key (plonk.hip plonk_check_witness_dev), under the context's lock
namespace mzk { struct WitnessCheckIn; }
// ... and registers a chunked proving key whose coefficient forms are resident on the device already (mzk_prover_create_from_circuit)
extern "C" int32_t mzk_ctx_pk_register_chunked(int32_t curve_id, uint32_t log_n, uint32_t num_wire_types, const void* selector_coeffs, const void* sigma_coeffs,
                                               const void* table_coeffs, uint64_t poly_len, const uint64_t* k_mont, const uint32_t* classes, uint32_t n_classes,
                                               int32_t coeffs_on_device, uint64_t* out_handle);
extern "C" int32_t mzk_ctx_check_witness(uint64_t pk_handle, const mzk::WitnessCheckIn* in, mzk_witness_report* out_report, void* stream);
// ... and derives the wire-variable table of a prover handle from its key's sigma coefficient forms (plonk.hip plonk_derive_variables_dev)
extern "C" int32_t mzk_ctx_derive_variables(uint64_t pk_handle, const void* d_sigma_coeffs, void* d_out_variables_u32, uint64_t* out_n_vars, void* stream);
// ... and encodes affine points in host memory as G1 records (the encoder of mzk_srs_serialize): the commitments of a serialized key
extern "C" int32_t mzk_ctx_g1_encode(int32_t curve_id, const uint64_t* xy_mont, uint64_t n_points, uint32_t flags, uint8_t* out_bytes);

namespace mzk {

void set_error(const std::string& s);

// hipSuccess -> MZK_OK; anything else sets "<what>: <HIP's message>" and maps to MZK_ERR_OOM / MZK_ERR_HIP
int32_t hip_status(hipError_t e, const char* what);

#define HIP_TRY(expr)                                      \
    do {                                                   \
        int32_t _r = ::mzk::hip_status((expr), #expr);     \
        if (_r != MZK_OK) return _r;                       \
    } while (0)

#define MZK_TRY(expr)                \
    do {                             \
        int32_t _r = (expr);         \
        if (_r != MZK_OK) return _r; \
    } while (0)

// grow-only device buffer
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int32_t reserve(size_t bytes);
    void release();
    template <class T> T* as() { return reinterpret_cast<T*>(p); }
};
// One device allocation that lives as long as a call or an object: move-only, allocated once, freed by the destructor.  The free
// happens on the device that is CURRENT then, so an owner dies only where its device is bound: inside the entry point that made it
// (ENTER_* in mzk.hip), under the DeviceGuard of the handle that owns it (verifier.hip), or in mzk_shutdown's per-context loop.
struct DevOwned {
    void* p = nullptr;
    DevOwned() = default;
    DevOwned(DevOwned&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevOwned& operator=(DevOwned&&) = delete;
    ~DevOwned() { if (p) (void)hipFree(p); }
    int32_t alloc(size_t bytes) { return hip_status(hipMalloc(&p, bytes ? bytes : 4), "hipMalloc"); }   // (0 bytes: still a valid pointer)
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct Workspace {
    DevBuf ntt_scratch, scalars, hist, offs, cursor, sorted, buckets, collect, io, misc, digits, long_desc, long_parts, plonk_polys, plonk_out, pre_cnt, pre_off, pre_ce, pre_cb, poly_tmp, split, link_tmp, occ, vid;
    void* h_collect = nullptr;
    size_t h_collect_cap = 0;
    double heavy_frac = 0.125;          // msm.hip: share of the worst case the heavy buckets' level-1 sums are sized for (grows on overflow, with a re-run)
    hipEvent_t last_use = nullptr;
    struct Named { const char* name; DevBuf Workspace::* buf; };
    static const Named bufs[];          // every DevBuf above with its name (mzk.hip): what release(), bytes() and the MZK_WS_DEBUG print walk
    void release();
    size_t bytes();
};

// every kernel launch of the library is counted (mzk_launch_count)
extern std::atomic<uint64_t> g_launches;
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, ...)                                  \
    do {                                                                     \
        ::mzk::g_launches.fetch_add(1, std::memory_order_relaxed);           \
        hipLaunchKernelGGLInternal((kernelName), __VA_ARGS__);               \
    } while (0)

// HIP-event timing of named regions (mzk_profile_*): one switch for the library, records per device context
extern std::atomic<bool> g_prof;                  // (switches shared by the device threads of one process: atomics)
struct ProfRec { std::string name; hipEvent_t a, b; };
struct ProfScope {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    const char* name;
    int logical = -1;                             // >= 0: the record goes to that context (taken under its lock), not to cur()
    ProfScope(const char* n, hipStream_t s);
    ProfScope(const char* n, hipStream_t s, int logical_device);   // for the translation units that run under a DeviceGuard, where cur() is not bound
    ~ProfScope();
};
extern std::atomic<bool> g_msm_precompute;

struct Srs {
    int curve = 0;
    uint64_t n = 0;
    uint32_t* d_xy = nullptr;   // n * 2 * fq words, boundary form (what mzk_srs_download returns)
    uint32_t* d_int = nullptr;  // internal reduced-radix table used by the MSM (R'-Montgomery form; BLS12-381: 13 signed 30-bit limbs in 14-word slots, ecz.cuh; BN254: 29-bit limbs, ecx.cuh)
    uint32_t* d_pre = nullptr;  // [W][n] precomputed multiples 2^(c*w) P_i (msm_pre.cuh), built on first large MSM
    int pre_c = 0;              // window bits of d_pre; -1 = do not build
    int pre_levels = 0;         // W: levels of d_pre
    double pre_build_ms = 0;    // wall time of the build (pre_next_level launches, synchronised)
    uint32_t* d_fk = nullptr;   // FK23 (kzg_multi.hip): the group NTT of [S_(fk_off + fk_d - 1) .. S_(fk_off), O^fk_d], 2 fk_d XYZZ points (EcFx form,
    uint64_t fk_off = 0, fk_d = 0;   // bit-reversed order) of the last (offset, d) a multi-opening asked for; built on first use
    void free();                // releases the tables (errors ignored) and nulls them; called explicitly, never from a destructor
};
inline bool valid_curve(int curve) { return curve == MZK_CURVE_BLS12_381 || curve == MZK_CURVE_BN254; }
inline int fq_words(int curve) { return curve == MZK_CURVE_BLS12_381 ? 12 : 8; }
inline size_t srs_point_bytes(int curve) { return (size_t)2 * fq_words(curve) * 4; }                            // boundary form (d_xy)
constexpr size_t srs_int_point_bytes(int curve) { return curve == MZK_CURVE_BLS12_381 ? 2 * 14 * 4 : 2 * 9 * 4; }  // internal form (d_int, d_pre): pinned to EcFz / EcFx::AFF_WORDS in msm.hip
constexpr size_t ec_ntt_point_bytes(int curve) { return curve == MZK_CURVE_BLS12_381 ? 4 * 14 * 4 : 4 * 9 * 4; }   // an XYZZ point of the group NTT (d_fk): pinned to EcFx::PT_WORDS in msm.hip

// ---- device contexts ---------------------------------------------------------------------------------
// One context per LOGICAL device: the HIP device it runs on, its lock, workspace, I/O slots, SRS registry; the NTT plan cache,
// the MSM sort streams and the proving keys are kept per context by their translation units (arrays indexed by Ctx::logical).
// A process may drive several devices, one host thread each (mzk_init(device) binds the calling thread; mzk_set_device rebinds
// it): calls on different contexts share nothing and run concurrently.  SRS / proving-key handles carry their context in the
// top 16 bits, so a handle-taking entry point needs no current device; entry points that take bare device pointers run on the
// calling thread's context (threads that never bound one use the first context initialised: the single-GPU case, Rayon workers
// included).  MZK_VIRTUAL_DEVICES=G maps logical devices 0..G-1 onto the physical ones round-robin -- G contexts on ONE card
// rehearse the multi-GPU code paths of a compiled host (mpc-jellyfish_amd/host/) on a one-GPU box.
constexpr int MAX_CTX = 16;
constexpr int IO_SLOTS = 4;
struct IoSlot {
    hipStream_t st = nullptr;
    DevBuf buf;
    bool busy = false;
};
struct Ctx {
    int logical = -1, device = -1;
    std::atomic<bool> init{false};                  // read without g_ctx_lock by the threads of other devices (handle look-ups)
    std::mutex lock;
    Workspace ws;
    std::vector<ProfRec> prof_recs;
    uint32_t last_c = 0, last_w = 0, last_m = 0;   // shape of the context's last MSM (mzk_msm_last_shape)
    uint32_t last_cap = 0, last_desc_cap = 0, last_h1_cap = 0, last_attempts = 0;   // rare-path sizing of its last MSM group (mzk_msm_last_rare)
    std::map<uint64_t, Srs> srs;
    uint64_t next_handle = 1;
    IoSlot io[IO_SLOTS];
    std::mutex io_lock;
    std::condition_variable io_cv;
};
Ctx& cur();                                       // the context the running entry point is bound to (thread-local)
// The shared workspace exists only inside a WsHold: acquire() makes `st` wait for the previous user's work, and the destructor
// records the event on `st` on EVERY return path, so what a failed call left queued stays covered.  Holds nest freely on one
// stream (a dispatch inside a hold takes its own).  ws_acquire / ws_release (mzk.hip) are the hold's two HIP calls: nothing else calls them.
int32_t ws_acquire(Workspace& ws, hipStream_t st);
void ws_release(Workspace& ws, hipStream_t st);
class WsHold {
    Workspace* ws_ = nullptr;                     // set once acquired: the workspace of the context that was current then
    hipStream_t st_ = nullptr;
   public:
    WsHold() = default;
    WsHold(const WsHold&) = delete;               // (no move either: one hold, one scope, one record)
    WsHold& operator=(const WsHold&) = delete;
    ~WsHold() { if (ws_) ws_release(*ws_, st_); }
    int32_t acquire(hipStream_t st) {
        Ctx& cx = cur();
        MZK_TRY(ws_acquire(cx.ws, st));
        ws_ = &cx.ws, st_ = st;
        return MZK_OK;
    }
    Workspace* operator->() const { return ws_; }
    Workspace& operator*() const { return *ws_; }
};
inline uint64_t handle_make(int logical, uint64_t counter) { return ((uint64_t)(logical + 1) << 48) | counter; }
inline int handle_ctx(uint64_t h) { return (int)(h >> 48) - 1; }
// the calling thread works on a handle's (logical) device for the duration of an entry point, for the translation units whose handles
// live outside Ctx (prover.hip, verifier.hip); the caller's own binding is back on return
struct DeviceGuard {
    int32_t prev = -1, rc = MZK_OK;
    bool switched = false;
    explicit DeviceGuard(int device) {
        if (mzk_get_device(&prev) != MZK_OK) prev = -1;
        if (prev != device) { rc = mzk_set_device(device); switched = rc == MZK_OK && prev >= 0; }
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
    ~DeviceGuard() { if (switched) (void)mzk_set_device(prev); }
};

// ntt.hip
// scale: 0 = boundary form in and out; 1 = output left in the internal form x * R' (R' = 2^261 = 32 R) of the quotient kernels;
// 2 = input in that form, output back in the boundary form (the factor rides in the final pass's multiplication)
// d_src (nullable): out of place -- the first pass reads the batch there (src_stride elements apart) and d_data only receives the result;
// d_patch (with d_src): 4 elements per batch entry that replace the input indices 0..3 (ntt_fx.cuh)
int32_t ntt_dispatch(int curve, uint32_t* d_data, uint64_t in_len, int log_n, bool inverse, const uint32_t* coset,
                     uint32_t batch, uint64_t stride, hipStream_t st, int scale = 0, const uint32_t* d_src = nullptr, uint64_t src_stride = 0,
                     const uint32_t* d_patch = nullptr, int skip_batch = -1 /* a batch entry that is not transformed */);
// The same transform over n_classes different cosets in ONE launch per pass (ntt_fx.cuh nttx_pass_classes_kernel): d_data holds
// n_classes * rows polynomials class-major, `stride` elements apart; with d_src every class reads the SAME rows of d_src (src_stride
// apart; d_patch class-major, 4 elements per entry).  2^10 <= N, n_classes <= 8; small transforms (the radix-2 pass form).
int32_t ntt_classes_dispatch(int curve, uint32_t* d_data, uint64_t in_len, int log_n, bool inverse, const uint32_t* const* cosets, int n_classes, uint32_t rows,
                             uint64_t stride, hipStream_t st, int scale, const uint32_t* d_src, uint64_t src_stride, const uint32_t* d_patch, int skip_batch);
void ntt_release_plans();
void msm_release_streams();
int32_t ctx_prover_stream(unsigned k, hipStream_t* out);      // msm.hip: a context-owned stream for a prover handle (never destroyed by the handle)
// msm.hip
int32_t msm_dispatch(const Srs& s, uint64_t base_offset, const uint32_t* d_scalars, uint64_t n, int is_mont, uint32_t* out, hipStream_t st);
int32_t msm_batch_dispatch(const Srs& s, uint32_t n_polys, const uint32_t* const* d_scalars, const uint64_t* lens, const uint64_t* base_offsets,
                           int is_mont, uint32_t* out_xyz, hipStream_t st);
int32_t srs_build_internal(Srs& s, hipStream_t st);
int32_t srs_build_pre(Srs& s, hipStream_t st);
int32_t srs_generate_dispatch(int curve, const uint32_t* beta_canon, const uint32_t* g_xy_mont /* NULL: the standard generator */, uint64_t n, uint32_t* d_out);
int32_t srs_lagrange_from_points_dispatch(int curve, const uint32_t* d_xy, int log_n, uint32_t n_extra, uint32_t* d_out);
// the group NTT (ec_ntt.cuh) of the 2^log_n XYZZ points at d_a (EcFx form), in place and asynchronous on st: natural order in, bit-reversed
// out; inverse: the root is w^-1; scaled: times 2^-log_n; d_tab: 8 points of scratch per butterfly (4 * 2^log_n, 8 at least).  d_out_xy
// (nullable): the finishing pass -- the first n_out elements in natural order as affine points in the boundary form, (0, 0) = infinity
int32_t ec_ntt_dispatch(int curve, uint32_t* d_a, int log_n, bool inverse, bool scaled, uint32_t* d_tab, uint32_t* d_out_xy, uint64_t n_out, hipStream_t st);
int32_t srs_lagrange_generate_dispatch(int curve, const uint32_t* beta_canon, const uint32_t* g_xy_mont /* nullable */, int log_n, uint32_t n_extra, uint32_t* d_out);
void jac_to_affine_host_dispatch(int curve, const uint64_t* xyz, uint64_t n, uint64_t* xy);
void jac_sum_host_dispatch(int curve, const uint64_t* xyz, uint64_t n, uint64_t* out);

// srs_io.hip: serialized G1 records (srs_io.cuh) <-> the boundary form of Srs::d_xy.  Decode reports the lowest failing index and the
// first check it failed (srs_bad_reason); *out_bad = ~0 when every point decoded.  Both run on `st`; decode synchronises it.
uint64_t srs_record_bytes(int curve, bool compressed);
const char* srs_bad_reason(int k);
int32_t srs_decode_dispatch(int curve, const uint8_t* d_in, uint64_t n, bool compressed, bool validate, uint32_t* d_xy, uint64_t* out_bad, int* out_reason,
                            hipStream_t st);
int32_t srs_encode_dispatch(int curve, const uint32_t* d_xy, uint64_t n, bool compressed, uint8_t* d_out, hipStream_t st);

// key_io.hip: the Fr records of a serialized key (key_io.cuh).  Decode: n_seg <= 32 segments of one staged image into rows of row_len
// aligned Montgomery elements, zero beyond a segment's count; *out_bad_seg / *out_bad_index = the lowest (segment, index) not below r, or
// all ones; synchronises st.  Arguments are validated by the entry points (mzk.hip).
int32_t fr_decode_dispatch(int curve, const uint8_t* d_image, uint32_t n_seg, const uint64_t* src, const uint64_t* count, const uint32_t* row, uint32_t* d_out,
                           uint64_t row_len, uint32_t* out_bad_seg, uint64_t* out_bad_index, hipStream_t st);
int32_t fr_encode_dispatch(int curve, const uint32_t* d_in, uint64_t n, uint32_t* d_out, hipStream_t st);

// poly.hip
int32_t poly_eval_dispatch(int curve, const uint32_t* d_coeffs, uint64_t stride, uint64_t len, uint32_t batch, const uint32_t* x_mont, uint32_t* out_host,
                           hipStream_t st);
struct EvalJob { const uint32_t* d; uint64_t len, stride; uint32_t batch, which_x; };
int32_t poly_eval_many_dispatch(int curve, const EvalJob* jobs, uint32_t n_jobs, const uint32_t* x_mont /* 2 x 8 words */, uint32_t* out_host, hipStream_t st);
int32_t poly_div_dispatch(int curve, const uint32_t* d_poly, uint64_t len, const uint32_t* z_mont, uint32_t* d_out, uint32_t* d_rem /* nullable: p(z) */, hipStream_t st);
// K openings in one pass: proofs to out_xy (host, affine), evaluations to out_evals (host); waits for the stream (its MSMs do)
int32_t kzg_open_batch_dispatch(const Srs& s, uint32_t K, const uint32_t* const* d_polys, const uint64_t* lens, const uint32_t* points_mont, uint64_t* out_xy,
                                uint32_t* out_evals, hipStream_t st);
int32_t poly_div_roots_dispatch(int curve, const uint32_t* d_poly, uint64_t len, uint32_t log_order, uint64_t first, uint64_t count, uint32_t* d_out,
                                hipStream_t st);
// kzg_multi.hip: mzk_kzg_multi_open_rou_dev behind its argument checks (either output nullable); waits for the stream
constexpr int KZG_MULTI_MAX_LOG = 21;       // cap on log2(2d) and log_domain (include/mzk.h: the workspace formula)
int32_t kzg_multi_open_dispatch(Srs& s, uint64_t srs_offset, const uint32_t* d_poly, uint64_t len, uint32_t log_domain, uint64_t num_points, uint64_t* out_xy,
                                uint32_t* out_evals, hipStream_t st);
// vid.hip: the ADVZ VID scheme behind its entry points' pointer checks (mzk_bytes_to_field_dev .. mzk_vid_advz_recover_dev); all but
// vid_bytes_to_field_dispatch wait for the stream
uint64_t vid_field_count(uint64_t len);                       // elements bytes_to_field makes of len bytes
int32_t vid_bytes_to_field_dispatch(int curve, const uint8_t* d_bytes, uint64_t len, uint32_t* d_out, hipStream_t st);
int32_t vid_field_to_bytes_dispatch(int curve, const uint32_t* d_elems, uint64_t count, uint8_t* d_out, uint64_t* out_len, hipStream_t st);
int32_t vid_commit_only_dispatch(Srs& s, uint64_t srs_offset, uint64_t srs_len, const uint32_t* d_elems, uint64_t n_elems, uint32_t k, uint32_t n, uint32_t log_domain,
                                 uint8_t* out_commit, hipStream_t st);
int32_t vid_disperse_dispatch(Srs& s, uint64_t srs_offset, uint64_t srs_len, const uint32_t* d_elems, uint64_t n_elems, uint32_t k, uint32_t n, uint32_t log_domain,
                              uint64_t* out_commits_xy, uint8_t* out_evals, uint64_t* out_proofs_xy, uint8_t* out_nodes, uint8_t* out_commit, uint8_t* out_root,
                              uint64_t* out_s_mont, hipStream_t st);
int32_t vid_verify_shares_dispatch(int curve, uint64_t S, uint64_t K, uint32_t n, const uint64_t* index, const uint8_t* evals, const uint8_t* paths, const uint8_t* root,
                                   const uint64_t* s_mont, int32_t* out_ok, uint64_t* out_agg_mont, hipStream_t st);
int32_t vid_recover_dispatch(int curve, uint32_t k, uint64_t K, uint32_t log_domain, const uint64_t* index, const uint64_t* y_mont, uint32_t* d_out, hipStream_t st);
int32_t poly_lincomb_dispatch(int curve, uint32_t n_terms, const uint32_t* const* d_polys, const uint64_t* lens, const uint32_t* scalars, uint32_t* d_out,
                              uint64_t out_len, hipStream_t st);
int32_t poly_degree_dispatch(const uint32_t* d_poly, uint64_t len, unsigned long long* d_out, hipStream_t st);
int32_t wire_gather_dispatch(const uint32_t* d_witness, uint64_t n_vars, const uint32_t* d_vars, uint64_t count, uint32_t* d_out, hipStream_t st);
int32_t poly_split_quotient_dispatch(int curve, const uint32_t* d_q, uint64_t n, uint32_t W, const uint32_t* blind_mont, uint32_t* d_out, uint64_t stride, hipStream_t st);
int32_t poly_mask_dispatch(int curve, uint32_t n_rows, uint32_t* const* d_rows, uint64_t n, uint32_t n_blind, const uint32_t* blind_mont, hipStream_t st);
// plonk.hip
int32_t plonk_pk_register(int curve, int log_n, int W, const uint32_t* sel, const uint32_t* sig, const uint32_t* tab /* NULL: TurboPlonk */,
                          uint64_t poly_len, const uint32_t* k_mont, const uint32_t* classes /* NULL: whole domain */, uint32_t n_classes,
                          uint64_t* out_handle, bool coeffs_on_device = false /* sel, sig, tab are device pointers */);
// the wire permutation of a variable table and its sigma values (perm.cuh)
int32_t plonk_wire_permutation_dev(const uint32_t* d_vars, uint64_t cells, uint64_t n_vars, uint32_t* d_next, hipStream_t st);
int32_t plonk_sigma_values_dev(int curve, int log_n, int W, const uint32_t* d_next, const uint32_t* k_mont, uint32_t* d_out, hipStream_t st);
// ... and the way back (unperm.cuh): sigma values -> permutation -> variables in canonical numbering; the three steps from a key's resident
// sigma coefficient forms (mzk_prover_derive_wire_variables)
int32_t plonk_sigma_decode_dev(int curve, int log_n, int W, const uint32_t* d_sigma, const uint32_t* k_mont, uint32_t* d_next, hipStream_t st);
int32_t plonk_variables_from_permutation_dev(const uint32_t* d_next, uint64_t cells, uint32_t* d_vars, uint64_t* out_n_vars, hipStream_t st);
int32_t plonk_derive_variables_dev(uint64_t handle, const uint32_t* d_sigma_coeffs, uint32_t* d_vars, uint64_t* out_n_vars, hipStream_t st);
int32_t plonk_quotient_chunked_dev(uint64_t handle, const uint32_t* d_polys, uint64_t in_stride, uint64_t in_len, uint32_t flags, const uint32_t* tau,
                                   const uint32_t* alpha, const uint32_t* beta, const uint32_t* gamma, uint32_t* d_out, hipStream_t st);
int32_t plonk_quotient_top_dev(uint64_t handle, const uint32_t* d_polys, uint64_t in_stride, uint64_t in_len, const uint32_t* alpha, const uint32_t* beta,
                               const uint32_t* gamma, uint32_t* d_top, uint32_t* out_n_top, hipStream_t st);
int32_t plonk_quotient_combine_dev(int curve, int log_n, const uint32_t* classes /* NULL: all 8 */, uint32_t n_classes, const uint32_t* d_r,
                                   const uint32_t* d_top /* nullable */, uint32_t n_top, uint32_t* d_out, hipStream_t st);
int32_t plonk_pk_release(uint64_t handle);
void plonk_release_all();
void verifier_release_all();                                  // verifier.hip: every verifier and open batch of the current context (mzk_shutdown)
int32_t plonk_quotient_dev(uint64_t handle, uint32_t* d_polys, uint64_t in_len, const uint32_t* tau /* NULL: TurboPlonk */, const uint32_t* alpha,
                           const uint32_t* beta, const uint32_t* gamma, uint32_t* d_out, hipStream_t st);
int32_t plookup_sorted_vec_dev(uint64_t handle, const uint32_t* d_wires, const uint32_t* tau, uint32_t* d_table, uint32_t* d_lookup, uint32_t* d_sorted,
                               hipStream_t st);
int32_t plookup_product_dev(uint64_t handle, const uint32_t* d_table, const uint32_t* d_lookup, const uint32_t* d_sorted, const uint32_t* beta,
                            const uint32_t* gamma, uint32_t* d_out, hipStream_t st);
// the witness check (check.cuh): the 13 selectors' coefficient forms (device, rows of n), the witness and the public input as
// mzk_prover_round1 takes them, the wire-variable table (device, nullable) -- validated by the caller (prover_check.inc)
struct WitnessCheckIn {
    const uint32_t* d_sel_coeffs;
    int kind;
    const void* witness;
    const uint32_t* d_vars;
    uint64_t n_vars;
    const uint64_t *pi_rows, *pi;
    uint64_t n_pi;
};
int32_t plonk_check_witness_dev(uint64_t handle, const WitnessCheckIn& in, mzk_witness_report* out, hipStream_t st);
int plonk_pk_is_ultra(uint64_t handle);
int32_t plonk_perm_product_dev(uint64_t handle, const uint32_t* d_wires, const uint32_t* beta, const uint32_t* gamma, uint32_t* d_out, hipStream_t st);
int plonk_pk_log_n(uint64_t handle);
int plonk_pk_curve(uint64_t handle);
int plonk_pk_classes(uint64_t handle, uint32_t* out);
int plonk_pk_wires(uint64_t handle);
uint64_t plonk_pk_bytes(uint64_t handle);

}  // namespace mzk
