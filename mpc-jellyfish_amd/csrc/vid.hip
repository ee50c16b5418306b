// vid.hip -- the ADVZ verifiable information dispersal scheme on the device (primitives/src/vid/advz.rs, Advz<E, Sha256>; DESIGN.md section
// 4.17): the launch sequences behind mzk_bytes_to_field_dev .. mzk_vid_advz_recover_dev (kernels: vid.cuh) and the host-only SHA-256 entry
// points (sha256.cuh).  disperse is two phases around ONE forced wait:
//   1  the K polynomials zero-padded into [K][N] -> the batched forward NTT (ntt.hip) -> the leaf kernel (evals[n][K] and n leaf digests from one read
//      of the NTT output) -> one launch per tree level -> the K commitments (msm_batch_dispatch over the payload as it lies: polynomial j is
//      elements j k .., the last one short)
//   -- the host: affine commitments, their uncompressed records (the encoder of mzk_srs_serialize), commit = SHA256(records),
//      s = hash_to_field(SHA256(records || root)) --
//   2  agg = s * sum_j poly_j -> FK23 (kzg_multi_open_dispatch) for the n proofs
// Scratch: Workspace::vid, one reservation per call (bytes: include/mzk.h); the dispatches called from here take their own buffers and holds.
#include <algorithm>
#include <string>
#include <vector>

#include "internal.hpp"
#include "hostfp.hpp"
#include "vid.cuh"

namespace mzk {
namespace {

constexpr char VID_DST[] = "rick";                                 // advz.rs:454 HASH_TO_FIELD_DOMAIN_SEP

inline unsigned grid_for(uint64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// 48 big-endian bytes mod r -> Montgomery words (from_be_bytes_mod_order)
template <class P>
void be_bytes_to_fr(const uint8_t* bytes, uint32_t n, uint32_t* out_mont) {
    using F = Fp64<P>;
    const F base = h64::from_u64<P>(256);
    F acc = F::zero();
    for (uint32_t i = 0; i < n; i++) acc = acc * base + h64::from_u64<P>(bytes[i]);
    acc.to_words(out_mont);
}
bool hash_to_field(int curve, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint64_t dst_len, uint32_t z_pad_len, uint32_t* out_mont) {
    uint8_t wide[sha256::HASH_TO_FIELD_BYTES];
    if (!sha256::expand_message_xmd(msg, len, dst, dst_len, z_pad_len, wide, sizeof wide)) return false;
    if (curve == MZK_CURVE_BLS12_381) be_bytes_to_fr<BlsFr>(wide, sizeof wide, out_mont);
    else be_bytes_to_fr<BnFr>(wide, sizeof wide, out_mont);
    return true;
}

template <class P>
void root_powers(uint32_t log_domain, const uint64_t* index, uint32_t k, uint32_t* out_mont) {
    const Fp64<P> w = h64::root_of_unity<P>((int)log_domain);
    for (uint32_t i = 0; i < k; i++) h64::pow_u64<P>(w, index[i]).to_words(out_mont + (size_t)i * 8);
}

// the tree over n leaves: level sizes from the leaves (level 0) up, `height` branch levels (advz.rs:325-338: ilog3(n) + 1)
struct TreeShape {
    uint32_t height = 0;
    uint64_t total = 0;
    std::vector<uint64_t> count, first;
};
TreeShape tree_shape(uint64_t n) {
    TreeShape t;
    for (uint64_t m = n; m >= 3; m /= 3) t.height++;
    t.height++;
    uint64_t c = n, at = 0;
    for (uint32_t l = 0; l <= t.height; l++) {
        t.count.push_back(c);
        t.first.push_back(at);
        at += c;
        c = (c + 2) / 3;
    }
    t.total = at;
    return t;
}

FrArg fr_arg_of(const uint32_t* mont) {
    FrArg a;
    std::memcpy(a.l, mont, sizeof a.l);
    return a;
}

struct Shape {
    uint64_t n_elems, K, N;
    uint32_t k, n, log_domain;
};
int32_t check_shape(const Srs& s, uint64_t srs_offset, uint64_t srs_len, uint64_t n_elems, uint32_t k, uint32_t n, uint32_t log_domain, Shape& sh) {
    const uint32_t two_adicity = s.curve == MZK_CURVE_BLS12_381 ? BlsFr::TWO_ADICITY : BnFr::TWO_ADICITY;
    if (k == 0 || n < k) { set_error("vid: payload_chunk_size " + std::to_string(k) + " is zero or exceeds num_storage_nodes " + std::to_string(n)); return MZK_ERR_INVALID_ARG; }
    if (log_domain > std::min<uint32_t>(two_adicity, KZG_MULTI_MAX_LOG)) { set_error("vid: log_domain above the two-adicity of the scalar field or the size cap of mzk_kzg_multi_open_rou_dev"); return MZK_ERR_UNSUPPORTED; }
    if (n > (1ull << log_domain) || k > (1ull << log_domain)) { set_error("vid: the domain holds fewer points than storage nodes"); return MZK_ERR_INVALID_ARG; }
    if (srs_offset > s.n || srs_len > s.n - srs_offset || k > srs_len) { set_error("vid: the SRS view holds fewer than payload_chunk_size points"); return MZK_ERR_INVALID_ARG; }
    if (n_elems >= (1ull << 40)) { set_error("vid: payload too long"); return MZK_ERR_INVALID_ARG; }
    sh = Shape{n_elems, (n_elems + k - 1) / k, 1ull << log_domain, k, n, log_domain};
    if (sh.K >= (1ull << 24)) { set_error("vid: more than 2^24 polynomials"); return MZK_ERR_UNSUPPORTED; }
    return MZK_OK;
}

// the K commitments of the payload's polynomials (host, affine), their uncompressed records, commit = SHA256(records).  Waits for the stream.
int32_t commit_phase(const Srs& s, uint64_t srs_offset, const uint32_t* d_elems, const Shape& sh, uint32_t* d_xy, uint8_t* d_rec, std::vector<uint64_t>& xy,
                     std::vector<uint8_t>& records, uint8_t* out_commit, hipStream_t st) {
    const size_t fw = fq_words(s.curve), rec = srs_record_bytes(s.curve, false);
    xy.assign(sh.K * fw, 0);                                       // (fw 32-bit words x 2 coordinates = fw 64-bit words per point)
    records.assign(sh.K * rec, 0);
    if (sh.K) {
        std::vector<const uint32_t*> ptr(sh.K);
        std::vector<uint64_t> lens(sh.K), offs(sh.K, srs_offset), jac(sh.K * 3 * fw / 2 + 1);
        for (uint64_t j = 0; j < sh.K; j++) {
            ptr[j] = d_elems + j * sh.k * 8;
            lens[j] = std::min<uint64_t>(sh.k, sh.n_elems - j * sh.k);
        }
        MZK_TRY(msm_batch_dispatch(s, (uint32_t)sh.K, ptr.data(), lens.data(), offs.data(), 1, reinterpret_cast<uint32_t*>(jac.data()), st));
        HIP_TRY(hipStreamSynchronize(st));
        jac_to_affine_host_dispatch(s.curve, jac.data(), sh.K, xy.data());
        HIP_TRY(hipMemcpyAsync(d_xy, xy.data(), sh.K * fw * 8, hipMemcpyHostToDevice, st));
        MZK_TRY(srs_encode_dispatch(s.curve, d_xy, sh.K, false, d_rec, st));
        HIP_TRY(hipMemcpyAsync(records.data(), d_rec, records.size(), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    sha256::digest(records.data(), records.size(), out_commit);
    return MZK_OK;
}

template <class P>
int32_t disperse_run(Srs& s, uint64_t srs_offset, const uint32_t* d_elems, const Shape& sh, uint64_t* out_commits_xy, uint8_t* out_evals, uint64_t* out_proofs_xy,
                     uint8_t* out_nodes, uint8_t* out_commit, uint8_t* out_root, uint64_t* out_s_mont, hipStream_t st) {
    const TreeShape tree = tree_shape(sh.n);
    const size_t fw = fq_words(s.curve), rec = srs_record_bytes(s.curve, false);
    const size_t ntt_bytes = sh.K * sh.N * 32, evals_bytes = (size_t)sh.n * sh.K * 32, nodes_bytes = tree.total * 32, agg_bytes = (size_t)sh.k * 32,
                 xy_bytes = sh.K * fw * 8, rec_bytes = sh.K * rec;
    WsHold ws; MZK_TRY(ws.acquire(st));
    MZK_TRY(ws->vid.reserve(ntt_bytes + evals_bytes + nodes_bytes + agg_bytes + xy_bytes + rec_bytes + 64));
    uint8_t* base = ws->vid.as<uint8_t>();
    uint32_t* d_ntt = reinterpret_cast<uint32_t*>(base);
    uint32_t* d_evals = reinterpret_cast<uint32_t*>(base + ntt_bytes);
    uint32_t* d_nodes = reinterpret_cast<uint32_t*>(base + ntt_bytes + evals_bytes);
    uint32_t* d_agg = reinterpret_cast<uint32_t*>(base + ntt_bytes + evals_bytes + nodes_bytes);
    uint32_t* d_xy = reinterpret_cast<uint32_t*>(base + ntt_bytes + evals_bytes + nodes_bytes + agg_bytes);
    uint8_t* d_rec = base + ntt_bytes + evals_bytes + nodes_bytes + agg_bytes + xy_bytes;
    std::vector<uint64_t> xy;
    std::vector<uint8_t> records;
    uint32_t s_mont[8];
    const auto run = [&]() -> int32_t {
        // phase 1: evaluate, hash, commit
        if (sh.K) {
            const uint64_t full = sh.n_elems / sh.k, rest = sh.n_elems % sh.k;
            HIP_TRY(hipMemsetAsync(d_ntt, 0, ntt_bytes, st));
            if (full) HIP_TRY(hipMemcpy2DAsync(d_ntt, sh.N * 32, d_elems, (size_t)sh.k * 32, (size_t)sh.k * 32, full, hipMemcpyDeviceToDevice, st));
            if (rest) HIP_TRY(hipMemcpyAsync(d_ntt + full * sh.N * 8, d_elems + full * sh.k * 8, rest * 32, hipMemcpyDeviceToDevice, st));
            for (uint64_t at = 0; at < sh.K; at += 32768) {        // (the batched NTT takes up to 65535 rows a call)
                const uint32_t rows = (uint32_t)std::min<uint64_t>(32768, sh.K - at);
                MZK_TRY(ntt_dispatch(s.curve, d_ntt + at * sh.N * 8, sh.k, (int)sh.log_domain, false, nullptr, rows, sh.N, st));
            }
        }
        hipLaunchKernelGGL((vid_leaf_kernel<P>), dim3(grid_for(sh.n, VID_LEAF_THREADS)), dim3(VID_LEAF_THREADS), 0, st, (const uint32_t*)d_ntt,
                           (unsigned long long)sh.N, (unsigned long long)sh.K, (unsigned long long)sh.n, d_evals, d_nodes);
        for (uint32_t l = 1; l <= tree.height; l++)
            hipLaunchKernelGGL(vid_branch_kernel, dim3(grid_for(tree.count[l], VID_LEAF_THREADS)), dim3(VID_LEAF_THREADS), 0, st,
                               (const uint32_t*)(d_nodes + tree.first[l - 1] * 8), (unsigned long long)tree.count[l - 1], d_nodes + tree.first[l] * 8,
                               (unsigned long long)tree.count[l]);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_nodes, d_nodes, nodes_bytes, hipMemcpyDeviceToHost, st));
        if (evals_bytes) HIP_TRY(hipMemcpyAsync(out_evals, d_evals, evals_bytes, hipMemcpyDeviceToHost, st));
        MZK_TRY(commit_phase(s, srs_offset, d_elems, sh, d_xy, d_rec, xy, records, out_commit, st));       // the one forced wait
        if (xy_bytes) std::memcpy(out_commits_xy, xy.data(), xy_bytes);
        std::memcpy(out_root, out_nodes + (tree.total - 1) * 32, 32);
        // the pseudorandom scalar: SHA256(records || root) through the field hasher
        uint8_t digest[32];
        sha256::Stream hs;
        if (!records.empty()) hs.update(records.data(), records.size());
        hs.update(out_root, 32);
        hs.finish(digest);
        if (!hash_to_field(s.curve, digest, 32, reinterpret_cast<const uint8_t*>(VID_DST), sizeof VID_DST - 1, sha256::XMD_Z_PAD_ARK, s_mont)) {
            set_error("vid: expand_message_xmd refused its arguments");
            return MZK_ERR_INVALID_ARG;
        }
        std::memcpy(out_s_mont, s_mont, 32);
        // phase 2: the aggregate polynomial and its n opening proofs
        if (sh.K)
            hipLaunchKernelGGL((vid_aggregate_kernel<P>), dim3(grid_for(sh.k, VID_THREADS)), dim3(VID_THREADS), 0, st, d_elems, (unsigned long long)sh.n_elems,
                               (unsigned long long)sh.k, fr_arg_of(s_mont), d_agg);
        HIP_TRY(hipGetLastError());
        return kzg_multi_open_dispatch(s, srs_offset, d_agg, sh.K ? sh.k : 0, sh.log_domain, sh.n, out_proofs_xy, nullptr, st);
    };
    const int32_t rc = run();
    const int32_t rs = hip_status(hipStreamSynchronize(st), "hipStreamSynchronize");      // (copies to the caller's memory may be queued on every path)
    return rc != MZK_OK ? rc : rs;
}

template <class P>
int32_t verify_run(int curve, uint64_t S, uint64_t K, uint32_t n, const uint64_t* index, const uint8_t* evals, const uint8_t* paths, const uint8_t* root,
                   const uint64_t* s_mont, int32_t* out_ok, uint64_t* out_agg_mont, hipStream_t st) {
    const TreeShape tree = tree_shape(n);
    const size_t idx_bytes = S * 8, ev_bytes = S * K * 32, path_bytes = S * tree.height * 64, ok_bytes = S * 4, agg_bytes = S * 32;
    const size_t at_ev = (idx_bytes + 31) & ~(size_t)31, at_path = at_ev + ev_bytes, at_root = at_path + path_bytes, at_agg = at_root + 32, at_ok = at_agg + agg_bytes;
    WsHold ws; MZK_TRY(ws.acquire(st));
    MZK_TRY(ws->vid.reserve(at_ok + ok_bytes + 64));
    uint8_t* base = ws->vid.as<uint8_t>();
    std::vector<uint32_t> ok(S);
    const auto run = [&]() -> int32_t {
        HIP_TRY(hipMemcpyAsync(base, index, idx_bytes, hipMemcpyHostToDevice, st));
        if (ev_bytes) HIP_TRY(hipMemcpyAsync(base + at_ev, evals, ev_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(base + at_path, paths, path_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(base + at_root, root, 32, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((vid_verify_kernel<P>), dim3(grid_for(S, VID_LEAF_THREADS)), dim3(VID_LEAF_THREADS), 0, st, reinterpret_cast<const unsigned long long*>(base),
                           reinterpret_cast<const uint32_t*>(base + at_ev), reinterpret_cast<const uint32_t*>(base + at_path),
                           reinterpret_cast<const uint32_t*>(base + at_root), (unsigned long long)S, (unsigned long long)K, (unsigned long long)n, tree.height,
                           fr_arg_of(reinterpret_cast<const uint32_t*>(s_mont)), reinterpret_cast<uint32_t*>(base + at_ok), reinterpret_cast<uint32_t*>(base + at_agg));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ok.data(), base + at_ok, ok_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_agg_mont, base + at_agg, agg_bytes, hipMemcpyDeviceToHost, st));
        return MZK_OK;
    };
    const int32_t rc = run();
    const int32_t rs = hip_status(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (rc == MZK_OK && rs == MZK_OK)
        for (uint64_t t = 0; t < S; t++) out_ok[t] = (int32_t)ok[t];
    return rc != MZK_OK ? rc : rs;
}

template <class P>
int32_t recover_run(uint32_t k, uint64_t K, uint32_t log_domain, const uint64_t* index, const uint64_t* y_mont, uint32_t* d_out, hipStream_t st) {
    const size_t x_bytes = (size_t)k * 32, m_bytes = (size_t)k * k * 32, y_bytes = K * k * 32;
    std::vector<uint32_t> x((size_t)k * 8);
    root_powers<P>(log_domain, index, k, x.data());
    WsHold ws; MZK_TRY(ws.acquire(st));
    MZK_TRY(ws->vid.reserve(2 * x_bytes + m_bytes + y_bytes + 64));
    uint32_t* d_x = ws->vid.as<uint32_t>();
    uint32_t* d_l = d_x + (size_t)k * 8;
    uint32_t* d_M = d_l + (size_t)k * 8;
    uint32_t* d_y = d_M + (size_t)k * k * 8;
    const auto run = [&]() -> int32_t {
        HIP_TRY(hipMemcpyAsync(d_x, x.data(), x_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_y, y_mont, y_bytes, hipMemcpyHostToDevice, st));
        const unsigned block = std::max(64u, (k + 63u) / 64u * 64u);
        hipLaunchKernelGGL((vid_master_kernel<P>), dim3(1), dim3(block), x_bytes, st, (const uint32_t*)d_x, k, d_l);
        hipLaunchKernelGGL((vid_rows_kernel<P>), dim3(grid_for(k, VID_THREADS)), dim3(VID_THREADS), 0, st, (const uint32_t*)d_x, (const uint32_t*)d_l, k, d_M);
        hipLaunchKernelGGL((vid_interpolate_kernel<P>), dim3(grid_for(K * k, VID_THREADS)), dim3(VID_THREADS), 0, st, (const uint32_t*)d_y, (const uint32_t*)d_M, k,
                           (unsigned long long)K, d_out);
        HIP_TRY(hipGetLastError());
        return MZK_OK;
    };
    const int32_t rc = run();
    const int32_t rs = hip_status(hipStreamSynchronize(st), "hipStreamSynchronize");      // (the uploads read the caller's and this frame's memory)
    return rc != MZK_OK ? rc : rs;
}

}  // namespace

uint64_t vid_field_count(uint64_t len) { return len / VID_ELEM_BYTES + (len % VID_ELEM_BYTES ? 2 : 0); }

int32_t vid_bytes_to_field_dispatch(int curve, const uint8_t* d_bytes, uint64_t len, uint32_t* d_out, hipStream_t st) {
    const uint64_t count = vid_field_count(len);
    if (!count) return MZK_OK;
    const dim3 grid(grid_for(count, VID_THREADS)), block(VID_THREADS);
    if (curve == MZK_CURVE_BLS12_381) hipLaunchKernelGGL((vid_bytes_to_field_kernel<BlsFr>), grid, block, 0, st, d_bytes, (unsigned long long)len, (unsigned long long)count, d_out);
    else hipLaunchKernelGGL((vid_bytes_to_field_kernel<BnFr>), grid, block, 0, st, d_bytes, (unsigned long long)len, (unsigned long long)count, d_out);
    return hip_status(hipGetLastError(), "vid_bytes_to_field_kernel");
}

int32_t vid_field_to_bytes_dispatch(int curve, const uint32_t* d_elems, uint64_t count, uint8_t* d_out, uint64_t* out_len, hipStream_t st) {
    *out_len = 0;
    if (!count) return MZK_OK;
    WsHold ws; MZK_TRY(ws.acquire(st));
    MZK_TRY(ws->vid.reserve(64));
    unsigned long long* d_len = ws->vid.as<unsigned long long>();
    const uint64_t writers = count > 1 ? count - 1 : count;
    const dim3 grid(grid_for(writers, VID_THREADS)), block(VID_THREADS);
    if (curve == MZK_CURVE_BLS12_381) hipLaunchKernelGGL((vid_field_to_bytes_kernel<BlsFr>), grid, block, 0, st, d_elems, (unsigned long long)count, d_out, d_len);
    else hipLaunchKernelGGL((vid_field_to_bytes_kernel<BnFr>), grid, block, 0, st, d_elems, (unsigned long long)count, d_out, d_len);
    int32_t rc = hip_status(hipGetLastError(), "vid_field_to_bytes_kernel");
    unsigned long long len = 0;
    if (rc == MZK_OK) rc = hip_status(hipMemcpyAsync(&len, d_len, sizeof len, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    const int32_t rs = hip_status(hipStreamSynchronize(st), "hipStreamSynchronize");
    *out_len = len;
    return rc != MZK_OK ? rc : rs;
}

int32_t vid_commit_only_dispatch(Srs& s, uint64_t srs_offset, uint64_t srs_len, const uint32_t* d_elems, uint64_t n_elems, uint32_t k, uint32_t n, uint32_t log_domain,
                                 uint8_t* out_commit, hipStream_t st) {
    Shape sh;
    MZK_TRY(check_shape(s, srs_offset, srs_len, n_elems, k, n, log_domain, sh));
    const size_t xy_bytes = sh.K * fq_words(s.curve) * 8, rec_bytes = sh.K * srs_record_bytes(s.curve, false);
    WsHold ws; MZK_TRY(ws.acquire(st));
    MZK_TRY(ws->vid.reserve(xy_bytes + rec_bytes + 64));
    std::vector<uint64_t> xy;
    std::vector<uint8_t> records;
    const int32_t rc = commit_phase(s, srs_offset, d_elems, sh, ws->vid.as<uint32_t>(), ws->vid.as<uint8_t>() + xy_bytes, xy, records, out_commit, st);
    const int32_t rs = hip_status(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc != MZK_OK ? rc : rs;
}

int32_t vid_disperse_dispatch(Srs& s, uint64_t srs_offset, uint64_t srs_len, const uint32_t* d_elems, uint64_t n_elems, uint32_t k, uint32_t n, uint32_t log_domain,
                              uint64_t* out_commits_xy, uint8_t* out_evals, uint64_t* out_proofs_xy, uint8_t* out_nodes, uint8_t* out_commit, uint8_t* out_root,
                              uint64_t* out_s_mont, hipStream_t st) {
    Shape sh;
    MZK_TRY(check_shape(s, srs_offset, srs_len, n_elems, k, n, log_domain, sh));
    if (s.curve == MZK_CURVE_BLS12_381)
        return disperse_run<BlsFr>(s, srs_offset, d_elems, sh, out_commits_xy, out_evals, out_proofs_xy, out_nodes, out_commit, out_root, out_s_mont, st);
    return disperse_run<BnFr>(s, srs_offset, d_elems, sh, out_commits_xy, out_evals, out_proofs_xy, out_nodes, out_commit, out_root, out_s_mont, st);
}

int32_t vid_verify_shares_dispatch(int curve, uint64_t S, uint64_t K, uint32_t n, const uint64_t* index, const uint8_t* evals, const uint8_t* paths, const uint8_t* root,
                                   const uint64_t* s_mont, int32_t* out_ok, uint64_t* out_agg_mont, hipStream_t st) {
    if (!S) return MZK_OK;
    if (n == 0 || S >= (1ull << 32) || K >= (1ull << 24)) { set_error("vid: no storage node, 2^32 shares or 2^24 evaluations a share"); return MZK_ERR_INVALID_ARG; }
    if (curve == MZK_CURVE_BLS12_381) return verify_run<BlsFr>(curve, S, K, n, index, evals, paths, root, s_mont, out_ok, out_agg_mont, st);
    return verify_run<BnFr>(curve, S, K, n, index, evals, paths, root, s_mont, out_ok, out_agg_mont, st);
}

int32_t vid_recover_dispatch(int curve, uint32_t k, uint64_t K, uint32_t log_domain, const uint64_t* index, const uint64_t* y_mont, uint32_t* d_out, hipStream_t st) {
    const uint32_t two_adicity = curve == MZK_CURVE_BLS12_381 ? BlsFr::TWO_ADICITY : BnFr::TWO_ADICITY;
    if (k == 0 || log_domain > two_adicity || log_domain > 63) { set_error("vid: payload_chunk_size zero or log_domain above the two-adicity of the scalar field"); return MZK_ERR_INVALID_ARG; }
    if (k > VID_RECOVER_MAX_K) {
        set_error("vid: recover takes payload_chunk_size up to " + std::to_string(VID_RECOVER_MAX_K) + " (the master polynomial is built in one workgroup)");
        return MZK_ERR_UNSUPPORTED;
    }
    if (K >= (1ull << 24)) { set_error("vid: more than 2^24 polynomials"); return MZK_ERR_UNSUPPORTED; }
    for (uint32_t i = 0; i < k; i++) {
        if (index[i] >> log_domain) { set_error("vid: share index " + std::to_string(index[i]) + " out of bounds for domain size " + std::to_string(1ull << log_domain)); return MZK_ERR_INVALID_ARG; }
        for (uint32_t j = 0; j < i; j++)
            if (index[i] == index[j]) { set_error("vid: duplicate input point at indices " + std::to_string(j) + ", " + std::to_string(i)); return MZK_ERR_INVALID_ARG; }
    }
    if (!K) return MZK_OK;
    if (curve == MZK_CURVE_BLS12_381) return recover_run<BlsFr>(k, K, log_domain, index, y_mont, d_out, st);
    return recover_run<BnFr>(k, K, log_domain, index, y_mont, d_out, st);
}

}  // namespace mzk

using namespace mzk;

// ---- host-only entry points: no kernel, no HIP call, no mzk_init ----
extern "C" int32_t mzk_sha256(const uint8_t* msg, uint64_t len, uint8_t* out32) {
    if (!out32 || (!msg && len)) { set_error("null pointer"); return MZK_ERR_INVALID_ARG; }
    sha256::digest(msg, len, out32);
    return MZK_OK;
}
extern "C" int32_t mzk_expand_message_xmd_sha256(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint64_t dst_len, uint32_t z_pad_len, uint8_t* out,
                                                 uint64_t out_len) {
    if ((!msg && len) || (!dst && dst_len) || (!out && out_len)) { set_error("null pointer"); return MZK_ERR_INVALID_ARG; }
    if (z_pad_len > 4096 || !sha256::expand_message_xmd(msg, len, dst, dst_len, z_pad_len, out, out_len)) {
        set_error("expand_message_xmd: at most 255 blocks and 65535 bytes out, a DST of at most 255 bytes, Z_pad of at most 4096");
        return MZK_ERR_INVALID_ARG;
    }
    return MZK_OK;
}
extern "C" int32_t mzk_hash_to_field_sha256(int32_t curve_id, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint64_t dst_len, uint64_t* out_mont) {
    if (!valid_curve(curve_id) || !out_mont || (!msg && len) || (!dst && dst_len)) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    if (!hash_to_field(curve_id, msg, len, dst, dst_len, sha256::XMD_Z_PAD_ARK, reinterpret_cast<uint32_t*>(out_mont))) {
        set_error("hash_to_field: a DST of at most 255 bytes");
        return MZK_ERR_INVALID_ARG;
    }
    return MZK_OK;
}
