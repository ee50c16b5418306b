// key_io.cuh -- Fr records of a serialized ProvingKey (ark-serialize 0.4: 32 bytes little-endian, the canonical integer, no flag bits;
// DESIGN.md section 4.13) <-> aligned Montgomery elements, one thread per element.  Memory-bound streaming: no LDS, coalesced access.
//
// Decode: one launch for a whole key.  The segment table travels by value (at most FR_MAX_SEGMENTS entries: the 13 + 5 / 14 + 6 + 4
// polynomials of a key and its k); grid.y is the segment, grid.x covers the row_len slots of its destination row.  A slot below the
// segment's count reads its record AT ANY BYTE ALIGNMENT -- everything after the is_merged byte of an image sits at odd offsets, so that
// is the normal case -- checks it is below r, converts with to_mont and writes an aligned element; a slot at or above the count writes
// zero (DensePolynomial strips trailing zeros; the prover's rows are n long).  The first failure is the lowest (segment, index) in segment
// order: a plain atomicMin on one 64-bit word preset to all ones, as srs_decode_kernel's.
#pragma once
#include <hip/hip_runtime.h>

#include "fp.cuh"
#include "srs_io.cuh"                                              // ser_below_modulus

namespace mzk {

constexpr int KEY_IO_THREADS = 256;
constexpr int FR_MAX_SEGMENTS = 32;
constexpr int FR_ERR_INDEX_BITS = 40;                            // err word = segment << 40 | index (row_len < 2^40)

struct FrSegments {
    unsigned long long src[FR_MAX_SEGMENTS];                     // byte offset of the first record in the staged image
    unsigned long long count[FR_MAX_SEGMENTS];                   // records (<= row_len)
    uint32_t row[FR_MAX_SEGMENTS];                               // destination row
};

// 32 bytes at p (any alignment) -> 8 little-endian words.  Aligned 4-byte loads over the 8 (p aligned) or 9 words the record touches,
// shifted into place; nothing outside the words that hold the record's own bytes is read.
MZK_D void fr_read_record(const uint8_t* __restrict__ p, uint32_t (&w)[8]) {
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u) * 8u;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - (sh >> 3));
    uint32_t v[9];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = q[j];
    v[8] = sh ? q[8] : 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = (uint32_t)((((uint64_t)v[j + 1] << 32) | v[j]) >> sh);
}

template <class P>
__global__ __launch_bounds__(KEY_IO_THREADS) void fr_decode_kernel(const uint8_t* __restrict__ image, FrSegments segs, uint32_t* __restrict__ out,
                                                                   unsigned long long row_len, unsigned long long* __restrict__ err) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t s = blockIdx.y;
    if (i >= row_len) return;
    Fp<P> a = Fp<P>::zero();
    if (i < segs.count[s]) {
        fr_read_record(image + segs.src[s] + i * 32ull, a.l);
        if (!ser_below_modulus<P>(a.l)) atomicMin(err, ((unsigned long long)s << FR_ERR_INDEX_BITS) | i);
        a = to_mont(a);                                          // (of a value not below r: garbage the host never uses)
    }
    store_fp<P>(out + ((unsigned long long)segs.row[s] * row_len + i) * 8ull, a);
}

template <class P>
__global__ __launch_bounds__(KEY_IO_THREADS) void fr_encode_kernel(const uint32_t* __restrict__ in, unsigned long long n, uint32_t* __restrict__ out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fp<P> a = from_mont(load_fp<P>(in + i * 8ull));
#pragma unroll
    for (int j = 0; j < 8; j++) out[i * 8ull + j] = a.l[j];       // (d_out is only 4-byte aligned: a section of an image under assembly)
}

}  // namespace mzk
