// srs_io.hip -- the kernels of mzk_srs_register_serialized[_dev] / mzk_srs_serialize (srs_io.cuh: formats and checks).
#include "internal.hpp"
#include "srs_io.cuh"

namespace mzk {

namespace {

constexpr int SRS_IO_THREADS = 256;

// err[k] = the lowest index whose FIRST failing check is k (plain atomicMin; SRS_BAD_REASONS entries, preset to ~0)
template <class X, bool COMPRESSED, bool VALIDATE>
__global__ __launch_bounds__(SRS_IO_THREADS) void srs_decode_kernel(const uint8_t* __restrict__ in, unsigned long long n, uint32_t* __restrict__ out_xy,
                                                                   unsigned long long* __restrict__ err) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int REC = (COMPRESSED ? 1 : 2) * SerFmt<X>::BYTES;
    const int bad = srs_decode_point<X, COMPRESSED, VALIDATE>(in + i * REC, out_xy + i * 2 * X::N);
    if (bad >= 0) atomicMin(&err[bad], i);
}

template <class X, bool COMPRESSED>
__global__ __launch_bounds__(SRS_IO_THREADS) void srs_encode_kernel(const uint32_t* __restrict__ xy, unsigned long long n, uint8_t* __restrict__ out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int REC = (COMPRESSED ? 1 : 2) * SerFmt<X>::BYTES;
    srs_encode_point<X, COMPRESSED>(xy + i * 2 * X::N, out + i * REC);
}

template <class X, bool COMPRESSED, bool VALIDATE>
void launch_decode(const uint8_t* d_in, uint64_t n, uint32_t* d_xy, unsigned long long* d_err, hipStream_t st) {
    hipLaunchKernelGGL((srs_decode_kernel<X, COMPRESSED, VALIDATE>), dim3((unsigned)((n + SRS_IO_THREADS - 1) / SRS_IO_THREADS)), dim3(SRS_IO_THREADS), 0,
                       st, d_in, (unsigned long long)n, d_xy, d_err);
}
template <class X>
void launch_decode_x(bool compressed, bool validate, const uint8_t* d_in, uint64_t n, uint32_t* d_xy, unsigned long long* d_err, hipStream_t st) {
    if (compressed) validate ? launch_decode<X, true, true>(d_in, n, d_xy, d_err, st) : launch_decode<X, true, false>(d_in, n, d_xy, d_err, st);
    else validate ? launch_decode<X, false, true>(d_in, n, d_xy, d_err, st) : launch_decode<X, false, false>(d_in, n, d_xy, d_err, st);
}

}  // namespace

uint64_t srs_record_bytes(int curve, bool compressed) {
    return (uint64_t)(curve == MZK_CURVE_BLS12_381 ? 48 : 32) * (compressed ? 1 : 2);
}

const char* srs_bad_reason(int k) {
    switch (k) {
        case SRS_BAD_FLAGS: return "invalid flag bits";
        case SRS_BAD_RANGE: return "coordinate not below the field modulus";
        case SRS_BAD_SQUARE: return "x^3 + b is not a square";
        case SRS_BAD_CURVE: return "not on the curve";
        case SRS_BAD_SUBGROUP: return "not in the subgroup";
        case SRS_BAD_INFINITY: return "point at infinity";
        default: return "?";
    }
}

int32_t srs_decode_dispatch(int curve, const uint8_t* d_in, uint64_t n, bool compressed, bool validate, uint32_t* d_xy, uint64_t* out_bad, int* out_reason,
                            hipStream_t st) {
    *out_bad = ~0ull;
    *out_reason = -1;
    if (!n) return MZK_OK;
    unsigned long long err[SRS_BAD_REASONS];
    DevOwned d_err;
    MZK_TRY(d_err.alloc(sizeof(err)));
    HIP_TRY(hipMemsetAsync(d_err.p, 0xFF, sizeof(err), st));
    if (curve == MZK_CURVE_BLS12_381) launch_decode_x<BlsFqX>(compressed, validate, d_in, n, d_xy, d_err.as<unsigned long long>(), st);
    else launch_decode_x<BnFqX>(compressed, validate, d_in, n, d_xy, d_err.as<unsigned long long>(), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < SRS_BAD_REASONS; k++)                     // a thread records only its first failing check: one reason holds the minimum
        if (err[k] < *out_bad) { *out_bad = err[k]; *out_reason = k; }
    return MZK_OK;
}

int32_t srs_encode_dispatch(int curve, const uint32_t* d_xy, uint64_t n, bool compressed, uint8_t* d_out, hipStream_t st) {
    if (!n) return MZK_OK;
    const dim3 grid((unsigned)((n + SRS_IO_THREADS - 1) / SRS_IO_THREADS)), block(SRS_IO_THREADS);
    if (curve == MZK_CURVE_BLS12_381) {
        if (compressed) hipLaunchKernelGGL((srs_encode_kernel<BlsFqX, true>), grid, block, 0, st, d_xy, (unsigned long long)n, d_out);
        else hipLaunchKernelGGL((srs_encode_kernel<BlsFqX, false>), grid, block, 0, st, d_xy, (unsigned long long)n, d_out);
    } else {
        if (compressed) hipLaunchKernelGGL((srs_encode_kernel<BnFqX, true>), grid, block, 0, st, d_xy, (unsigned long long)n, d_out);
        else hipLaunchKernelGGL((srs_encode_kernel<BnFqX, false>), grid, block, 0, st, d_xy, (unsigned long long)n, d_out);
    }
    HIP_TRY(hipGetLastError());
    return MZK_OK;
}

}  // namespace mzk
