// When may a staged single-chunk encode run the column kernel's dense entry
// (rs_mono.hip k_mono_dense, rs_device.hpp MonoLeadDense)?  Decided on the host from
// the launch's row maps and shard format; plain C++ (no device headers), so that
// tests/mono_dense_check.cpp can compile it alone.
#pragma once
#include <cstdint>

namespace rs {

// One row map of the launch: transform row r in [row_begin, row_end) at
// base + (r - row_begin) * stride.
struct DenseRows {
    const void *base;
    uint64_t stride;
    uint32_t row_begin, row_end;
};

// The dense entry addresses a lane's rows as a wave-uniform 64-bit base plus one
// 32-bit lane offset, row * stride + byte offset inside the row (< stride), formed by
// a 24-bit multiply.  Bound: stride < 2^24 and 2^L * stride <= 2^32, so every offset
// of rows [0, 2^L) fits 32 bits.  (A batch adds stripe * stripe stride to the uniform
// base in 64 bits: no bound on the stripe strides.)
inline bool mono_dense_stride_ok(int L, uint64_t stride) {
    return stride < (uint64_t(1) << 24) && (stride << L) <= (uint64_t(1) << 32);
}

// nsrc source maps (src: the first), the destination map, the ShardFormat's three
// fields, and the stripe strides of a batch (0 for one stripe).  True: rows [0, 2^L)
// all lie in src and in dst, every pack is a full one (shards of whole 64-byte
// blocks), and every row of every stripe starts 4-byte aligned.
inline bool mono_dense_ok(int L, uint32_t nsrc, const DenseRows &src, const DenseRows &dst, uint32_t full_packs,
                          uint32_t tail_h, uint32_t io_bytes, uint64_t src_bstride = 0, uint64_t dst_bstride = 0) {
    if (L < 7 || L > 11 || nsrc != 1) return false;
    if (full_packs != 0xFFFFFFFFu || tail_h != 0 || io_bytes != 0) return false;
    const uint32_t n = 1u << L;
    if (src.row_begin != 0 || src.row_end < n || dst.row_begin != 0 || dst.row_end < n) return false;
    if (((uintptr_t(src.base) | src.stride | src_bstride | uintptr_t(dst.base) | dst.stride | dst_bstride) & 3u) != 0)
        return false;
    return mono_dense_stride_ok(L, src.stride) && mono_dense_stride_ok(L, dst.stride);
}

}  // namespace rs
