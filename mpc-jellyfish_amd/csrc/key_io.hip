// key_io.hip -- the kernels of mzk_fr_decode_dev / mzk_fr_encode_dev (key_io.cuh) and the host-only container parser behind
// mzk_key_layout (keyfmt.hpp): what mzk_prover_create_serialized / mzk_prover_serialize_key (prover.hip) are made of.
#include "internal.hpp"
#include "key_io.cuh"
#include "keyfmt.hpp"

namespace mzk {

int32_t fr_decode_dispatch(int curve, const uint8_t* d_image, uint32_t n_seg, const uint64_t* src, const uint64_t* count, const uint32_t* row, uint32_t* d_out,
                           uint64_t row_len, uint32_t* out_bad_seg, uint64_t* out_bad_index, hipStream_t st) {
    *out_bad_seg = ~0u;
    *out_bad_index = ~0ull;
    if (!n_seg || !row_len) return MZK_OK;
    FrSegments segs{};
    for (uint32_t s = 0; s < n_seg; s++) { segs.src[s] = src[s]; segs.count[s] = count[s]; segs.row[s] = row[s]; }
    unsigned long long err = ~0ull;
    DevOwned d_err;
    MZK_TRY(d_err.alloc(sizeof(err)));
    HIP_TRY(hipMemsetAsync(d_err.p, 0xFF, sizeof(err), st));
    const dim3 grid((unsigned)((row_len + KEY_IO_THREADS - 1) / KEY_IO_THREADS), n_seg), block(KEY_IO_THREADS);
    if (curve == MZK_CURVE_BLS12_381) hipLaunchKernelGGL((fr_decode_kernel<BlsFr>), grid, block, 0, st, d_image, segs, d_out, (unsigned long long)row_len, d_err.as<unsigned long long>());
    else hipLaunchKernelGGL((fr_decode_kernel<BnFr>), grid, block, 0, st, d_image, segs, d_out, (unsigned long long)row_len, d_err.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (err != ~0ull) {
        *out_bad_seg = (uint32_t)(err >> FR_ERR_INDEX_BITS);
        *out_bad_index = err & ((1ull << FR_ERR_INDEX_BITS) - 1);
    }
    return MZK_OK;
}

int32_t fr_encode_dispatch(int curve, const uint32_t* d_in, uint64_t n, uint32_t* d_out, hipStream_t st) {
    if (!n) return MZK_OK;
    const dim3 grid((unsigned)((n + KEY_IO_THREADS - 1) / KEY_IO_THREADS)), block(KEY_IO_THREADS);
    if (curve == MZK_CURVE_BLS12_381) hipLaunchKernelGGL((fr_encode_kernel<BlsFr>), grid, block, 0, st, d_in, (unsigned long long)n, d_out);
    else hipLaunchKernelGGL((fr_encode_kernel<BnFr>), grid, block, 0, st, d_in, (unsigned long long)n, d_out);
    HIP_TRY(hipGetLastError());
    return MZK_OK;
}

}  // namespace mzk

using namespace mzk;

extern "C" int32_t mzk_key_layout(int32_t curve_id, const uint8_t* bytes, uint64_t len, uint32_t flags, mzk_key_layout_t* out) {
    if (!valid_curve(curve_id) || !out || (!bytes && len)) { set_error("bad argument"); return MZK_ERR_INVALID_ARG; }
    keyfmt::Walk w(bytes, len);
    if (keyfmt::walk(w, curve_id, flags, out)) return MZK_OK;
    set_error(w.err);
    return MZK_ERR_ENCODING;
}
