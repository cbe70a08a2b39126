// Kernels of a verify (rs_verify_device*, DESIGN.md "Verify"): do the recovery
// shards of a stripe still agree with its originals?
//
//   k_mono_verify   the fused route: the staged single-chunk column encode whose
//                   store_col loads the caller's word from the address it would
//                   store to, compares, and flags the row on a difference
//                   (rs_device.hpp MonoVerifyArgs, launch_mono_verify).  The body
//                   is rs_mono.hip's; this translation unit builds only its verify
//                   instantiations, rs_mono.hip's own object none of them, so the
//                   encode's kernels stay as they were.
//   k_verify_rows   the unfused route's compare: the encode in scratch against
//                   the caller's rows over a row list (launch_verify_rows)
//   k_mono_verify_masks, k_verify_rows_masks   the two with a selection per stripe
//                   (rs_verify_device_batch_masks)
#define RS_MONO_VERIFY_TU 1
#include "rs_mono.hip"

namespace rs {
namespace {

// One thread per pack of one row; blockIdx.y = entry of the row list, blockIdx.z
// = stripe.  Lanes that find a difference all store the same byte to the row's
// flag: plain byte stores, no atomics.
__global__ __launch_bounds__(256) void k_verify_rows(const VerifyRowsArgs A) {
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (pk >= A.packs || r >= A.nrows) return;
    const PackIO io = pack_io(A.fmt, pk);
    const uint32_t j = A.rows ? A.rows[r] : r;
    const uint64_t b = blockIdx.z;
    const uint8_t *w = A.want + b * A.want_bstride + uint64_t(j) * A.want_stride + io.lo;
    const uint8_t *h = A.have + b * A.have_bstride + uint64_t(j) * A.have_stride + io.lo;
    const uint32_t wl = ld_word(w, io), wh = ld_word(w + io.hi_delta, io);
    const uint32_t hl = ld_word(h, io), hh = ld_word(h + io.hi_delta, io);
    if (wl != hl || wh != hh) A.flags[b * A.flag_bstride + j] = 1;
}

// k_verify_rows with stripe b's own row list (rs_device.hpp VerifyRowsMaskArgs).  The
// grid's y is the batch's largest count: a workgroup past its stripe's count leaves
// after one scalar load, before any row is addressed.
__global__ __launch_bounds__(256) void k_verify_rows_masks(const VerifyRowsMaskArgs A) {
    const uint64_t b = blockIdx.z;
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (r >= A.counts[b] || pk >= A.packs) return;
    const PackIO io = pack_io(A.fmt, pk);
    const uint32_t j = A.rows[b * A.list_stride + r];
    const uint8_t *w = A.want + b * A.want_bstride + uint64_t(j) * A.want_stride + io.lo;
    const uint8_t *h = A.have + b * A.have_bstride + uint64_t(j) * A.have_stride + io.lo;
    const uint32_t wl = ld_word(w, io), wh = ld_word(w + io.hi_delta, io);
    const uint32_t hl = ld_word(h, io), hh = ld_word(h + io.hi_delta, io);
    if (wl != hl || wh != hh) A.flags[b * A.flag_bstride + j] = 1;
}

}  // namespace

hipError_t launch_verify_rows_masks(const VerifyRowsMaskArgs &A, hipStream_t s) {
    if (!A.packs || !A.nrows || !A.stripes) return hipSuccess;
    if (A.nrows > 65535 || A.stripes > 65535 || !A.rows || !A.counts) return hipErrorInvalidValue;
    const uint32_t threads = A.packs >= 256 ? 256u : (A.packs + 63u) / 64u * 64u;
    k_verify_rows_masks<<<dim3((A.packs + threads - 1) / threads, A.nrows, A.stripes), threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_verify_rows_masks");
    return hipGetLastError();
}

hipError_t launch_verify_rows(const VerifyRowsArgs &A, hipStream_t s) {
    if (!A.packs || !A.nrows || !A.stripes) return hipSuccess;
    if (A.nrows > 65535 || A.stripes > 65535) return hipErrorInvalidValue;
    const uint32_t threads = A.packs >= 256 ? 256u : (A.packs + 63u) / 64u * 64u;
    k_verify_rows<<<dim3((A.packs + threads - 1) / threads, A.nrows, A.stripes), threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_verify_rows");
    return hipGetLastError();
}

}  // namespace rs
