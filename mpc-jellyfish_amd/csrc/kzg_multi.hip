// kzg_multi.hip -- UnivariatePCS::multi_open_rou on the device: the opening proofs of ONE polynomial at every point of a radix-2 domain by
// FK23 (https://eprint.iacr.org/2023/033 section 2.2; the reference's compute_h_poly_in_fk23, univariate_kzg/mod.rs:336-376, and
// ToeplitzMatrix::fast_vec_mul, toeplitz.rs:118-140), and its evaluations there by one scalar NTT.  DESIGN.md section 4.16.
//
// The proof at x is [q_x(beta)]g, q_x = (f - f(x)) / (X - x) = sum_i h_i(beta) x^i with h_i = sum_(j >= i) f_(d - (j - i)) beta^(d - 1 - j): the h_i are
// a Toeplitz matrix of coefficients times the SRS vector s = [S_(d-1), .., S_0], and the proofs are the polynomial sum_i [h_i] X^i evaluated
// on the domain.  The Toeplitz product is a cyclic convolution of size 2d (circulant embedding):
//   A  s^ = NTT_2d([S_(d-1), .., S_0, O^d])                    group NTT (ec_ntt.cuh); depends on the SRS alone: kept on its handle (Srs::d_fk)
//   B  c^ = NTT_2d([f_d, 0^(d-1), f_d, f_1, .., f_(d-1)])       the scalar NTT (ntt.hip), natural order
//   C  u^_k = (c^_k / 2d) s^_k                                  2d scalar multiplications, one thread each (fk_pointwise_kernel)
//   D  u = 2d NTT^-1_2d(u^); h = u[0 .. d)                       group NTT, unscaled: the 1 / 2d rode in step C
//   E  proofs = NTT_N([h, O^(N - d)])[0 .. num_points)          group NTT with the finishing pass (affine, boundary form)
// Index orders: the group NTT takes natural order and leaves bit-reversed order, so s^ sits bit-reversed (position p holds s^_bitrev(p)); step
// C reads c^ at bitrev(p) and WRITES u^ at bitrev(p), which is the natural order step D wants; step D leaves h bit-reversed, and the kernel that
// pads h with N - d points at infinity for step E -- needed anyway, N being the caller's -- reads it at bitrev(i).  No permutation pass.
#include <algorithm>
#include <string>

#include "internal.hpp"
#include "ec_ntt.cuh"
#include "poly.cuh"

namespace mzk {
namespace {

__device__ __forceinline__ unsigned long long bit_reverse(unsigned long long i, int log_n) {
    unsigned long long r = 0;
    for (int b = 0; b < log_n; b++) r |= ((i >> b) & 1ull) << (log_n - 1 - b);
    return r;
}

// the circulant column (step B's input), 2d Montgomery elements; f_k = 0 from len on
__global__ __launch_bounds__(POLY_THREADS) void fk_column_kernel(const uint32_t* __restrict__ poly, unsigned long long len, unsigned long long d,
                                                                 uint32_t* __restrict__ col) {
    const unsigned long long i = (unsigned long long)blockIdx.x * POLY_THREADS + threadIdx.x;
    if (i >= 2 * d) return;
    const unsigned long long k = (i == 0 || i == d) ? d : (i > d ? i - d : len);         // (len: none, a zero)
#pragma unroll
    for (int q = 0; q < 8; q++) col[i * 8 + q] = k < len ? poly[k * 8 + q] : 0u;
}

// step C.  s_hat, u: n XYZZ points; c_hat: n Montgomery elements in natural order; tab: 8 points for each of the n threads
template <class FR, class X>
__global__ __launch_bounds__(EC_NTT_THREADS) void fk_pointwise_kernel(const uint32_t* __restrict__ s_hat, const uint32_t* __restrict__ c_hat, unsigned long long n,
                                                                      int log_n, FrArg scale_mont, uint32_t* __restrict__ u, uint32_t* __restrict__ tab) {
    using EC = EcFx<X>;
    const unsigned long long p = (unsigned long long)blockIdx.x * EC_NTT_THREADS + threadIdx.x;
    if (p >= n) return;
    const unsigned long long k = bit_reverse(p, log_n);
    const Fp<FR> c = from_mont(load_fp<FR>(c_hat + k * 8) * fr_arg<FR>(scale_mont));
    uint32_t kk[8];
#pragma unroll
    for (int q = 0; q < 8; q++) kk[q] = c.l[q];
    EC::store_pt(u, k, ecx_scalar_mul<X>(EC::load_pt(s_hat, p), kk, tab, p, n));
}

// step E's input: e[i] = h_i = u[bitrev(i)] (u: step D's output of size 2^log_m) for i < d, infinity for d <= i < n
template <class X>
__global__ __launch_bounds__(EC_NTT_THREADS) void fk_pad_kernel(const uint32_t* __restrict__ u, int log_m, unsigned long long d, unsigned long long n,
                                                                uint32_t* __restrict__ e) {
    using EC = EcFx<X>;
    const unsigned long long i = (unsigned long long)blockIdx.x * EC_NTT_THREADS + threadIdx.x;
    if (i >= n) return;
    EC::store_pt(e, i, i < d ? EC::load_pt(u, bit_reverse(i, log_m)) : XYZZX<X>::inf());
}

// step A on a handle that does not hold it for (off, d): the former table goes first
template <class X>
int32_t build_s_hat(Srs& s, uint64_t off, uint64_t d, int log_m, uint32_t* tab, hipStream_t st) {
    using EC = EcFx<X>;
    const uint64_t m = 2 * d;
    if (s.d_fk) (void)hipFree(s.d_fk);
    s.d_fk = nullptr;
    s.fk_d = 0;
    uint32_t* a = nullptr;
    HIP_TRY(hipMalloc((void**)&a, m * EC::PT_WORDS * 4));
    hipLaunchKernelGGL((ecx_ntt_load_kernel<X>), dim3((unsigned)((m + EC_NTT_THREADS - 1) / EC_NTT_THREADS)), dim3(EC_NTT_THREADS), 0, st,
                       (const uint32_t*)(s.d_xy + off * 2 * X::N), (unsigned long long)m, a, (unsigned long long)d, true);
    int32_t rc = ec_ntt_dispatch(s.curve, a, log_m, false, false, tab, nullptr, 0, st);
    if (rc == MZK_OK) rc = hip_status(hipStreamSynchronize(st), "hipStreamSynchronize (FK23 SRS transform)");
    if (rc != MZK_OK) { (void)hipFree(a); return rc; }
    s.d_fk = a, s.fk_off = off, s.fk_d = d;
    return MZK_OK;
}

template <class FR, class X>
int32_t multi_open_run(Srs& s, uint64_t off, const uint32_t* d_poly, uint64_t len, int log_d, int log_domain, uint64_t num_points, uint64_t* out_xy,
                       uint32_t* out_evals, hipStream_t st) {
    using EC = EcFx<X>;
    const uint64_t N = 1ull << log_domain, d = 1ull << log_d, m = 2 * d;
    const int log_m = log_d + 1;
    const bool proofs = out_xy && len > 1;
    const size_t xy_bytes = (size_t)2 * X::N * 4;
    if (out_xy && !proofs) std::memset(out_xy, 0, num_points * xy_bytes);              // a constant (or no) polynomial: the zero witness
    WsHold ws; MZK_TRY(ws.acquire(st));
    // Everything is reserved before anything is queued, and every path below waits for the stream: a copy to the caller's memory may be on it.
    // scalars: the evaluations (N elements), then -- the copy to the host queued -- the circulant column (2d) in the same place; the affine proofs behind
    const size_t fr_elems = std::max<uint64_t>(out_evals ? N : 0, proofs ? m : 0);
    MZK_TRY(ws->poly_tmp.reserve(fr_elems * 32 + (proofs ? num_points * xy_bytes : 0) + 32));
    // points: u (2d), e (N) and the window tables -- 8 points per thread of step C (2d threads) or of a stage of step E (N / 2) -- a peak that is
    // handed back below when this call had to grow the workspace for it, as the Lagrange key does (srs_lagrange_from_points)
    const size_t parts_before = ws->long_parts.cap, parts_need = proofs ? (m + N + 8 * std::max(m, N / 2) + 8) * EC::PT_WORDS * 4 : 0;
    MZK_TRY(ws->long_parts.reserve(parts_need));
    uint32_t* fr = ws->poly_tmp.as<uint32_t>();
    uint32_t* d_xy_out = fr + fr_elems * 8;
    uint32_t* u = ws->long_parts.as<uint32_t>();
    uint32_t* e = u + m * EC::PT_WORDS;
    uint32_t* tab = e + N * EC::PT_WORDS;
    const auto run = [&]() -> int32_t {
        if (out_evals) {
            if (len) HIP_TRY(hipMemcpyAsync(fr, d_poly, len * 32, hipMemcpyDeviceToDevice, st));
            if (len < N) HIP_TRY(hipMemsetAsync(fr + len * 8, 0, (N - len) * 32, st));
            MZK_TRY(ntt_dispatch(s.curve, fr, N, log_domain, false, nullptr, 1, N, st));
            HIP_TRY(hipMemcpyAsync(out_evals, fr, num_points * 32, hipMemcpyDeviceToHost, st));
        }
        if (!proofs) return MZK_OK;
        if (!(s.d_fk && s.fk_off == off && s.fk_d == d)) MZK_TRY(build_s_hat<X>(s, off, d, log_m, tab, st));
        hipLaunchKernelGGL(fk_column_kernel, dim3((unsigned)((m + POLY_THREADS - 1) / POLY_THREADS)), dim3(POLY_THREADS), 0, st, d_poly, (unsigned long long)len,
                           (unsigned long long)d, fr);
        MZK_TRY(ntt_dispatch(s.curve, fr, m, log_m, false, nullptr, 1, m, st));
        const unsigned gm = (unsigned)((m + EC_NTT_THREADS - 1) / EC_NTT_THREADS), gN = (unsigned)((N + EC_NTT_THREADS - 1) / EC_NTT_THREADS);
        hipLaunchKernelGGL((fk_pointwise_kernel<FR, X>), dim3(gm), dim3(EC_NTT_THREADS), 0, st, (const uint32_t*)s.d_fk, (const uint32_t*)fr, (unsigned long long)m,
                           log_m, to_fr_arg<FR>(inv(from_u64<FR>(m))), u, tab);
        MZK_TRY(ec_ntt_dispatch(s.curve, u, log_m, true, false, tab, nullptr, 0, st));
        hipLaunchKernelGGL((fk_pad_kernel<X>), dim3(gN), dim3(EC_NTT_THREADS), 0, st, (const uint32_t*)u, log_m, (unsigned long long)d, (unsigned long long)N, e);
        MZK_TRY(ec_ntt_dispatch(s.curve, e, log_domain, false, false, tab, d_xy_out, num_points, st));
        HIP_TRY(hipMemcpyAsync(out_xy, d_xy_out, num_points * xy_bytes, hipMemcpyDeviceToHost, st));
        return MZK_OK;
    };
    const int32_t rc = run();
    const int32_t rs = hip_status(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (parts_before < parts_need) ws->long_parts.release();
    return rc != MZK_OK ? rc : rs;
}

}  // namespace

int32_t kzg_multi_open_dispatch(Srs& s, uint64_t srs_offset, const uint32_t* d_poly, uint64_t len, uint32_t log_domain, uint64_t num_points, uint64_t* out_xy,
                                uint32_t* out_evals, hipStream_t st) {
    const bool bls = s.curve == MZK_CURVE_BLS12_381;
    const uint32_t max_log = std::min<uint32_t>(bls ? BlsFr::TWO_ADICITY : BnFr::TWO_ADICITY, KZG_MULTI_MAX_LOG);
    if (log_domain > max_log) {
        set_error("multi_open_rou: log_domain above the two-adicity of the scalar field or the size cap of " + std::to_string(KZG_MULTI_MAX_LOG));
        return MZK_ERR_UNSUPPORTED;
    }
    const uint64_t N = 1ull << log_domain, top = len ? len - 1 : 0;
    int log_d = 0;                                                 // d = next_power_of_two(max(len, 1) - 1), next_power_of_two(0) = 1
    while (log_d < 63 && (1ull << log_d) < top) log_d++;
    const uint64_t d = 1ull << log_d;
    if (out_evals && len > N) {
        set_error("multi_open_rou: a polynomial with " + std::to_string(len) + " coefficients can't be evaluated on a smaller domain with size " + std::to_string(N));
        return MZK_ERR_INVALID_ARG;
    }
    if (out_xy) {
        if ((uint32_t)log_d + 1 > max_log) {
            set_error("multi_open_rou: 2d above the two-adicity of the scalar field or the size cap of 2^" + std::to_string(KZG_MULTI_MAX_LOG));
            return MZK_ERR_UNSUPPORTED;
        }
        if (srs_offset > s.n || d > s.n - srs_offset) {
            set_error("multi_open_rou: the SRS view holds fewer than d = " + std::to_string(d) + " points");
            return MZK_ERR_INVALID_ARG;
        }
        if (d > N) {
            set_error("multi_open_rou: d = " + std::to_string(d) + " proof coefficients can't be evaluated on a smaller domain with size " + std::to_string(N));
            return MZK_ERR_INVALID_ARG;
        }
    }
    if (num_points > N) num_points = N;
    if (num_points == 0 || (!out_xy && !out_evals)) return MZK_OK;
    if (bls) return multi_open_run<BlsFr, BlsFqX>(s, srs_offset, d_poly, len, log_d, (int)log_domain, num_points, out_xy, out_evals, st);
    return multi_open_run<BnFr, BnFqX>(s, srs_offset, d_poly, len, log_d, (int)log_domain, num_points, out_xy, out_evals, st);
}

}  // namespace mzk
