// vid.cuh -- the kernels of the ADVZ verifiable information dispersal scheme (primitives/src/vid/advz.rs, Advz<E, Sha256>; DESIGN.md
// section 4.17).  Everything here is one thread per output with the field element in registers; SHA-256 comes from sha256.cuh with static
// schedule indices only.  Launch sequences and scratch: vid.hip.
//   bytes <-> field   utilities/src/conversion.rs:379-523 as written (31 bytes per element, the length element, its quirk at multiples of 31)
//   leaf              node i < n reads evaluation [j][i] of the NTT output for j = 0 .. K - 1 (neighbouring threads, neighbouring addresses),
//                     writes it canonical to evals[i][j] and hashes the same words: SHA256(u64_le(i) || u64_le(K) || K x 32 bytes)
//   branch            one level of the ternary tree: SHA256(c0 || c1 || c2), 32 zero bytes for a missing child
//   aggregate         agg[c] = s * sum_j a[j k + c]: the reference's polynomial_eval is `coeff * point + res` -- point times the SUM
//   verify            one thread per share: the leaf from the share's evaluations, the climb with the index's base-3 digits, s * sum_j eval_j
//   recover           the k x k matrix of the Lagrange basis on the shares' points (master polynomial in one workgroup; l'(x_i), one inversion
//                     and a synthetic division per row), then out[p][c] = sum_i y[p][i] M[i][c]
#pragma once
#include <hip/hip_runtime.h>

#include "fp.cuh"
#include "fp_inv.cuh"
#include "poly.cuh"                                                // FrArg
#include "sha256.cuh"

namespace mzk {

constexpr int VID_THREADS = 256;
constexpr int VID_LEAF_THREADS = 64;                              // few, long threads: n storage nodes, K elements each
constexpr uint32_t VID_ELEM_BYTES = 31;                           // conversion.rs compile_time_checks: (MODULUS_BIT_SIZE - 1) / 8 on both curves
constexpr uint32_t VID_RECOVER_MAX_K = 1024;                      // the master polynomial lives in one workgroup (vid_master_kernel)

// ---- bytes -> field ---------------------------------------------------------------------------------------------------------------------
// count = len / 31 (+ 2 when 31 does not divide len: the zero-extended last group, then its byte count).  Any alignment of `bytes`.
template <class P>
__global__ __launch_bounds__(VID_THREADS) void vid_bytes_to_field_kernel(const uint8_t* __restrict__ bytes, unsigned long long len, unsigned long long count,
                                                                         uint32_t* __restrict__ out) {
    const unsigned long long e = (unsigned long long)blockIdx.x * VID_THREADS + threadIdx.x;
    if (e >= count) return;
    const unsigned long long full = len / VID_ELEM_BYTES;
    const uint32_t rem = (uint32_t)(len % VID_ELEM_BYTES);
    Fp<P> a = Fp<P>::zero();
    if (e > full) {
        a.l[0] = rem;                                              // the length element, written by the thread that owns it
    } else {
        const uint32_t nb = e < full ? VID_ELEM_BYTES : rem;
        const uint8_t* p = bytes + e * VID_ELEM_BYTES;
#pragma unroll
        for (uint32_t b = 0; b < VID_ELEM_BYTES; b++)              // (static limb indices: the element stays in registers)
            if (b < nb) a.l[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    }
    store_fp<P>(out + e * 8ull, to_mont(a));                       // (below 2^248: canonical as it stands)
}

// ---- field -> bytes ---------------------------------------------------------------------------------------------------------------------
// FieldToBytes as written: one element -> its low 31 bytes; otherwise elements 0 .. count - 3 give 31 bytes each and element count - 2 gives
// min(low 64 bits of element count - 1, 32) of its 32 bytes.  The thread of element count - 2 (or of the only element) writes *out_len.
template <class P>
__global__ __launch_bounds__(VID_THREADS) void vid_field_to_bytes_kernel(const uint32_t* __restrict__ elems, unsigned long long count, uint8_t* __restrict__ out,
                                                                         unsigned long long* __restrict__ out_len) {
    const unsigned long long e = (unsigned long long)blockIdx.x * VID_THREADS + threadIdx.x;
    const unsigned long long writers = count > 1 ? count - 1 : count;
    if (e >= writers) return;
    const Fp<P> a = from_mont(load_fp<P>(elems + e * 8ull));
    uint32_t nb = VID_ELEM_BYTES;
    if (count > 1 && e == count - 2) {
        const Fp<P> last = from_mont(load_fp<P>(elems + (count - 1) * 8ull));
        nb = (last.l[1] != 0u || last.l[0] > 32u) ? 32u : last.l[0];
        *out_len = (count - 2) * VID_ELEM_BYTES + nb;
    } else if (count == 1) {
        *out_len = VID_ELEM_BYTES;
    }
    uint8_t* p = out + e * VID_ELEM_BYTES;
#pragma unroll
    for (uint32_t b = 0; b < 32; b++)
        if (b < nb) p[b] = (uint8_t)(a.l[b >> 2] >> (8 * (b & 3)));
}

// ---- the leaf digest ----------------------------------------------------------------------------------------------------------------------
// SHA256(u64_le(pos) || u64_le(K) || elem_0 || .. || elem_(K-1)), elem(j) giving element j as its 8 canonical little-endian words.  The
// header takes words 0..3 of the first block; even elements land on words 4..11, odd ones straddle two blocks: every index is static, and the
// message ends at word 12 (K odd) or 4 (K even).  Digest: the words of its bytes in memory.
template <class Elem>
MZK_D void vid_leaf_digest(unsigned long long pos, unsigned long long K, Elem elem, uint32_t (&out)[8]) {
    uint32_t h[8], w[16], a[8];
    sha256::init(h);
    w[0] = sha256::bswap((uint32_t)pos); w[1] = sha256::bswap((uint32_t)(pos >> 32));
    w[2] = sha256::bswap((uint32_t)K);   w[3] = sha256::bswap((uint32_t)(K >> 32));
    const unsigned long long total = 16ull + 32ull * K;
    unsigned long long j = 0;
#pragma unroll 1
    for (; j + 1 < K; j += 2) {
        elem(j, a);
#pragma unroll
        for (int q = 0; q < 8; q++) w[4 + q] = sha256::bswap(a[q]);
        elem(j + 1, a);
#pragma unroll
        for (int q = 0; q < 4; q++) w[12 + q] = sha256::bswap(a[q]);
        sha256::compress(h, w);
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = sha256::bswap(a[4 + q]);
    }
    if (j < K) {
        elem(j, a);
#pragma unroll
        for (int q = 0; q < 8; q++) w[4 + q] = sha256::bswap(a[q]);
        sha256::finish_words<12>(h, w, total);
    } else {
        sha256::finish_words<4>(h, w, total);
    }
#pragma unroll
    for (int q = 0; q < 8; q++) out[q] = sha256::bswap(h[q]);
}

// ntt: [K][N] Montgomery evaluations; evals: [n][K] canonical; nodes: n digests
template <class P>
__global__ __launch_bounds__(VID_LEAF_THREADS) void vid_leaf_kernel(const uint32_t* __restrict__ ntt, unsigned long long N, unsigned long long K, unsigned long long n,
                                                                     uint32_t* __restrict__ evals, uint32_t* __restrict__ nodes) {
    const unsigned long long i = (unsigned long long)blockIdx.x * VID_LEAF_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t d[8];
    vid_leaf_digest(i, K, [&](unsigned long long j, uint32_t (&a)[8]) {
        const Fp<P> v = from_mont(load_fp<P>(ntt + (j * N + i) * 8ull));
        store_fp<P>(evals + (i * K + j) * 8ull, v);
#pragma unroll
        for (int q = 0; q < 8; q++) a[q] = v.l[q];
    }, d);
#pragma unroll
    for (int q = 0; q < 8; q++) nodes[i * 8ull + q] = d[q];
}

// one level: parent p = SHA256 of children 3p, 3p + 1, 3p + 2, zeros from n_child on
__global__ __launch_bounds__(VID_LEAF_THREADS) void vid_branch_kernel(const uint32_t* __restrict__ child, unsigned long long n_child, uint32_t* __restrict__ parent,
                                                                       unsigned long long n_parent) {
    const unsigned long long p = (unsigned long long)blockIdx.x * VID_LEAF_THREADS + threadIdx.x;
    if (p >= n_parent) return;
    uint32_t c[3][8], d[8];
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int q = 0; q < 8; q++) c[t][q] = 3 * p + t < n_child ? child[(3 * p + t) * 8ull + q] : 0u;
    sha256::hash_branch(c[0], c[1], c[2], d);
#pragma unroll
    for (int q = 0; q < 8; q++) parent[p * 8ull + q] = d[q];
}

// ---- aggregate ------------------------------------------------------------------------------------------------------------------------------
// elems: the payload's n_elems Montgomery elements, polynomial j = elements j k .. ; out[c] = s * sum_j elems[j k + c], c < k
template <class P>
__global__ __launch_bounds__(VID_THREADS) void vid_aggregate_kernel(const uint32_t* __restrict__ elems, unsigned long long n_elems, unsigned long long k, FrArg s_mont,
                                                                    uint32_t* __restrict__ out) {
    const unsigned long long c = (unsigned long long)blockIdx.x * VID_THREADS + threadIdx.x;
    if (c >= k) return;
    Fp<P> acc = Fp<P>::zero();
#pragma unroll 1
    for (unsigned long long at = c; at < n_elems; at += k) acc = acc + load_fp<P>(elems + at * 8ull);
    store_fp<P>(out + c * 8ull, acc * fr_arg<P>(s_mont));
}

// ---- verify ---------------------------------------------------------------------------------------------------------------------------------
// share t: index[t], evals[t][K] canonical, path[t][height][2] sibling digests (the two other children of each level, in order; zeros for an
// empty one).  ok[t] = 1 when the digests climb to `root`; agg[t] = s * sum_j evals[t][j] (Montgomery).
template <class P>
__global__ __launch_bounds__(VID_LEAF_THREADS) void vid_verify_kernel(const unsigned long long* __restrict__ index, const uint32_t* __restrict__ evals,
                                                                       const uint32_t* __restrict__ path, const uint32_t* __restrict__ root, unsigned long long S,
                                                                       unsigned long long K, unsigned long long n, uint32_t height, FrArg s_mont,
                                                                       uint32_t* __restrict__ ok, uint32_t* __restrict__ agg) {
    const unsigned long long t = (unsigned long long)blockIdx.x * VID_LEAF_THREADS + threadIdx.x;
    if (t >= S) return;
    unsigned long long idx = index[t];
    Fp<P> acc = Fp<P>::zero();
    uint32_t cur[8];
    vid_leaf_digest(idx, K, [&](unsigned long long j, uint32_t (&a)[8]) {
        const Fp<P> v = load_fp<P>(evals + (t * K + j) * 8ull);
        acc = acc + to_mont(v);
#pragma unroll
        for (int q = 0; q < 8; q++) a[q] = v.l[q];
    }, cur);
    bool good = idx < n;
#pragma unroll 1
    for (uint32_t l = 0; l < height; l++) {
        const uint32_t digit = (uint32_t)(idx % 3ull);
        idx /= 3ull;
        const uint32_t* sib = path + ((t * height + l) * 2ull) * 8ull;
        uint32_t c[3][8], d[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t s0 = sib[q], s1 = sib[8 + q];
            c[0][q] = digit == 0 ? cur[q] : s0;
            c[1][q] = digit == 1 ? cur[q] : (digit == 0 ? s0 : s1);
            c[2][q] = digit == 2 ? cur[q] : s1;
        }
        sha256::hash_branch(c[0], c[1], c[2], d);
#pragma unroll
        for (int q = 0; q < 8; q++) cur[q] = d[q];
    }
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) diff |= cur[q] ^ root[q];
    ok[t] = (good && idx == 0 && diff == 0) ? 1u : 0u;
    store_fp<P>(agg + t * 8ull, acc * fr_arg<P>(s_mont));
}

// ---- recover --------------------------------------------------------------------------------------------------------------------------------
// l(X) = prod_i (X - x_i), coefficients 0 .. k - 1 (it is monic of degree k: the top one is not stored).  ONE workgroup of >= k threads,
// thread j keeps coefficient j in registers; step i is l_j <- l_(j-1) - x_i l_j, the neighbour's value through LDS (k * 32 bytes).
template <class P>
__global__ __launch_bounds__(VID_RECOVER_MAX_K) void vid_master_kernel(const uint32_t* __restrict__ x, uint32_t k, uint32_t* __restrict__ l) {
    extern __shared__ uint32_t vid_sh[];
    const uint32_t j = threadIdx.x;
    Fp<P> cur = j == 0 ? Fp<P>::one() : Fp<P>::zero();
#pragma unroll 1
    for (uint32_t i = 0; i < k; i++) {
        if (j < k) {
#pragma unroll
            for (int q = 0; q < 8; q++) vid_sh[q * k + j] = cur.l[q];
        }
        __syncthreads();
        Fp<P> prev = Fp<P>::zero();
        if (j > 0 && j < k) {
#pragma unroll
            for (int q = 0; q < 8; q++) prev.l[q] = vid_sh[q * k + j - 1];
        }
        if (j < k) cur = prev - load_fp<P>(x + i * 8ull) * cur;
        __syncthreads();
    }
    if (j < k) store_fp<P>(l + j * 8ull, cur);
}

// row i of M: w_i l(X) / (X - x_i), w_i = 1 / l'(x_i) = 1 / prod_(j != i) (x_i - x_j); the quotient by synthetic division from the top
template <class P>
__global__ __launch_bounds__(VID_THREADS) void vid_rows_kernel(const uint32_t* __restrict__ x, const uint32_t* __restrict__ l, uint32_t k, uint32_t* __restrict__ M) {
    const uint32_t i = blockIdx.x * VID_THREADS + threadIdx.x;
    if (i >= k) return;
    const Fp<P> xi = load_fp<P>(x + i * 8ull);
    Fp<P> d = Fp<P>::one();
#pragma unroll 1
    for (uint32_t j = 0; j < k; j++)
        if (j != i) d = d * (xi - load_fp<P>(x + j * 8ull));
    const Fp<P> w = inv_safegcd<P>(d);
    Fp<P> li = Fp<P>::one();
    store_fp<P>(M + ((unsigned long long)i * k + (k - 1)) * 8ull, w);
#pragma unroll 1
    for (uint32_t c = k - 1; c-- > 0;) {
        li = load_fp<P>(l + (c + 1) * 8ull) + xi * li;
        store_fp<P>(M + ((unsigned long long)i * k + c) * 8ull, w * li);
    }
}

// out[p][c] = sum_i y[p][i] M[i][c]: K k threads, neighbouring c read neighbouring addresses of a row of M
template <class P>
__global__ __launch_bounds__(VID_THREADS) void vid_interpolate_kernel(const uint32_t* __restrict__ y, const uint32_t* __restrict__ M, uint32_t k, unsigned long long K,
                                                                      uint32_t* __restrict__ out) {
    const unsigned long long t = (unsigned long long)blockIdx.x * VID_THREADS + threadIdx.x;
    if (t >= K * k) return;
    const unsigned long long p = t / k, c = t % k;
    Fp<P> acc = Fp<P>::zero();
#pragma unroll 1
    for (uint32_t i = 0; i < k; i++) acc = acc + load_fp<P>(y + (p * k + i) * 8ull) * load_fp<P>(M + ((unsigned long long)i * k + c) * 8ull);
    store_fp<P>(out + t * 8ull, acc);
}

}  // namespace mzk
