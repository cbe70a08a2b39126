// Kernels of a partial-stripe write (rs_update_device*, DESIGN.md "Update").
//
// The encode is GF(2^16)-linear per column, so overwriting originals index[c],
// c < count, changes recovery row j by XOR_c G[j][c] * (old_c ^ new_c), where
// G[j][c] is element c of recovery row j of the encode of the unit stripe
// (row index[c] holds the element 1 at column c, everything else zero).
//
//   k_coef_unit / k_coef_log   the coefficient step around that encode: the unit
//                              stripe in, log G[j][c] out (once per index list)
//   k_update                   the direct route: recovery_j ^= XOR_c delta_c * G[j][c]
//   k_update_lists             the same with an index list and a row selection per stripe,
//                              the logs read from the table over every original
//   k_rows_xor                 out = a ^ b over a row list: the two ends of the
//                              re-encode route (delta stripe in, recovery rows out)
#include <cstdio>

#include "rs_device.hpp"
#include "rs_gf.hpp"

namespace rs {
namespace {

// A load through the constant address space from a wave-uniform address goes
// through the scalar cache into SGPRs: one table fetch per wave, not per lane.
typedef const __attribute__((address_space(4))) uint32_t *ConstWords;
__device__ __forceinline__ ConstWords const_words(const void *p) {
    return (ConstWords)(reinterpret_cast<uintptr_t>(p));
}

constexpr int kTableWords = 20;  // words of one perm table (gf_tables.hpp kPermWords)

__global__ void k_coef_unit(uint8_t *unit, uint64_t stride, const uint32_t *index, uint32_t count) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    unit[uint64_t(index[c]) * stride + (c >> 5) * 64u + (c & 31u)] = 1;
}

__global__ void k_coef_log(const uint8_t *coef, uint64_t stride, uint32_t rows, uint32_t count,
                           const uint16_t *log_table, uint16_t *logs) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (c >= count || j >= rows) return;
    const uint8_t *p = coef + uint64_t(j) * stride + (c >> 5) * 64u + (c & 31u);
    logs[uint64_t(j) * count + c] = log_table[uint32_t(p[0]) | uint32_t(p[32]) << 8];  // log[0] = kUpdateNoCoef
}

// One thread per pack; blockIdx.y = group of rows_per_group selected recovery
// rows, blockIdx.z = stripe.  Row numbers, logs and tables are wave-uniform.
template <bool OLD>
__global__ __launch_bounds__(256) void k_update(const UpdateArgs A) {
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = pk < A.packs;
    const PackIO io = pack_io(A.fmt, ok ? pk : 0u);
    const uint64_t stripe = blockIdx.z;
    const uint8_t *nw = A.new_rows + stripe * A.new_bstride + io.lo;
    const uint8_t *od = OLD ? A.old_rows + stripe * A.old_bstride + io.lo : nullptr;
    uint8_t *rec = A.rec + stripe * A.rec_bstride + io.lo;
    const ConstWords logs = const_words(A.logs), lut = const_words(A.lut), rows = const_words(A.rows);

    uint32_t dl[kUpdateTile], dh[kUpdateTile];
    auto load_tile = [&](uint32_t c0) {
        static_for<0, int(kUpdateTile)>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const uint32_t c = c0 + uint32_t(i);
            dl[i] = dh[i] = 0;
            if (c < A.count && ok) {
                const uint8_t *p = nw + uint64_t(c) * A.new_stride;
                dl[i] = ld_word(p, io);
                dh[i] = ld_word(p + io.hi_delta, io);
                if constexpr (OLD) {
                    const uint8_t *q = od + uint64_t(c) * A.old_stride;
                    dl[i] ^= ld_word(q, io);
                    dh[i] ^= ld_word(q + io.hi_delta, io);
                }
            }
        });
    };
    const bool single = A.count <= kUpdateTile;  // the deltas stay in registers across the rows
    if (single) load_tile(0);

    const uint32_t r0 = blockIdx.y * A.rows_per_group;
    const uint32_t r1 = r0 + A.rows_per_group < A.nsel ? r0 + A.rows_per_group : A.nsel;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t j = A.rows ? rows[r] : r;
        uint32_t al = 0, ah = 0;
        for (uint32_t c0 = 0; c0 < A.count; c0 += kUpdateTile) {
            if (!single) load_tile(c0);
            static_for<0, int(kUpdateTile)>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const uint32_t c = c0 + uint32_t(i);
                if (c < A.count) {
                    const uint32_t e = j * A.count + c;
                    const uint32_t lg =
                        __builtin_amdgcn_readfirstlane((logs[e >> 1] >> ((e & 1u) * 16u)) & 0xFFFFu);
                    if (lg != kUpdateNoCoef) {  // a zero coefficient: nothing to add
                        uint32_t t[kTableWords];
#pragma unroll
                        for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(lg) * kTableWords + w];
                        gf_muladd4(al, ah, dl[i], dh[i], t);
                    }
                }
            });
        }
        if (ok) {
            uint8_t *p = rec + uint64_t(j) * A.rec_stride;
            st_word(p, ld_word(p, io) ^ al, io);
            st_word(p + io.hi_delta, ld_word(p + io.hi_delta, io) ^ ah, io);
        }
    }
}

// k_update with one index list and one row selection per stripe (rs_update_device_batch_lists).
// The logs come from the table over every original (pitch A.N), so the scalar chain is
// index -> log -> perm table.  The indices are fetched beside the deltas: once per workgroup
// for a count <= kUpdateTile, with every tile of every row above it (as k_update reloads its
// deltas there).  blockIdx.y = group of rows_per_group recovery rows of A.M.
template <bool OLD>
__global__ __launch_bounds__(256) void k_update_lists(const UpdateListsArgs A) {
    const uint64_t stripe = blockIdx.z;
    const uint32_t count = const_words(A.counts)[stripe];
    if (!count) return;  // an empty list, or a stripe the launch leaves out
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = pk < A.packs;
    const PackIO io = pack_io(A.fmt, ok ? pk : 0u);
    const uint8_t *nw = A.new_rows + stripe * A.new_bstride + io.lo;
    const uint8_t *od = OLD ? A.old_rows + stripe * A.old_bstride + io.lo : nullptr;
    uint8_t *rec = A.rec + stripe * A.rec_bstride + io.lo;
    const ConstWords logs = const_words(A.logs), lut = const_words(A.lut), sel = const_words(A.sel);
    const ConstWords index = const_words(A.index + stripe * A.index_pitch);

    uint32_t dl[kUpdateTile], dh[kUpdateTile], ix[kUpdateTile];
    auto load_tile = [&](uint32_t c0) {
        static_for<0, int(kUpdateTile)>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const uint32_t c = c0 + uint32_t(i);
            dl[i] = dh[i] = ix[i] = 0;
            if (c < count) {
                ix[i] = index[c];
                if (ok) {
                    const uint8_t *p = nw + uint64_t(c) * A.new_stride;
                    dl[i] = ld_word(p, io);
                    dh[i] = ld_word(p + io.hi_delta, io);
                    if constexpr (OLD) {
                        const uint8_t *q = od + uint64_t(c) * A.old_stride;
                        dl[i] ^= ld_word(q, io);
                        dh[i] ^= ld_word(q + io.hi_delta, io);
                    }
                }
            }
        });
    };
    const bool single = count <= kUpdateTile;  // the deltas and indices stay in registers across the rows
    if (single) load_tile(0);

    const uint32_t r0 = blockIdx.y * A.rows_per_group;
    const uint32_t r1 = r0 + A.rows_per_group < A.M ? r0 + A.rows_per_group : A.M;
    const uint32_t sel0 = uint32_t(stripe) * A.M;  // (at most 65535 stripes of at most 65536 rows)
    for (uint32_t j = r0; j < r1; ++j) {
        if (A.sel) {
            const uint32_t e = sel0 + j;
            if (!((sel[e >> 2] >> ((e & 3u) * 8u)) & 0xFFu)) continue;  // not selected: the row is never touched
        }
        uint32_t al = 0, ah = 0;
        for (uint32_t c0 = 0; c0 < count; c0 += kUpdateTile) {
            if (!single) load_tile(c0);
            static_for<0, int(kUpdateTile)>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const uint32_t c = c0 + uint32_t(i);
                if (c < count) {
                    const uint32_t e = j * A.N + ix[i];
                    const uint32_t lg =
                        __builtin_amdgcn_readfirstlane((logs[e >> 1] >> ((e & 1u) * 16u)) & 0xFFFFu);
                    if (lg != kUpdateNoCoef) {  // a zero coefficient: nothing to add
                        uint32_t t[kTableWords];
#pragma unroll
                        for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(lg) * kTableWords + w];
                        gf_muladd4(al, ah, dl[i], dh[i], t);
                    }
                }
            });
        }
        if (ok) {
            uint8_t *p = rec + uint64_t(j) * A.rec_stride;
            st_word(p, ld_word(p, io) ^ al, io);
            st_word(p + io.hi_delta, ld_word(p + io.hi_delta, io) ^ ah, io);
        }
    }
}

__global__ __launch_bounds__(256) void k_rows_xor(const UpdateXorArgs A) {
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (pk >= A.packs || r >= A.nrows) return;
    const PackIO io = pack_io(A.fmt, pk);
    const uint32_t lr = A.list ? A.list[r] : r;
    const uint8_t *a = A.a + uint64_t(A.a_list ? lr : r) * A.a_stride + io.lo;
    uint32_t l = ld_word(a, io), h = ld_word(a + io.hi_delta, io);
    if (A.b) {
        const uint8_t *b = A.b + uint64_t(A.b_list ? lr : r) * A.b_stride + io.lo;
        l ^= ld_word(b, io);
        h ^= ld_word(b + io.hi_delta, io);
    }
    uint8_t *o = A.out + uint64_t(A.out_list ? lr : r) * A.out_stride + io.lo;
    st_word(o, l, io);
    st_word(o + io.hi_delta, h, io);
}

uint32_t block_threads(uint32_t packs) { return packs >= 256 ? 256u : (packs + 63u) / 64u * 64u; }

}  // namespace

hipError_t launch_update_unit(uint8_t *unit, uint64_t stride, const uint32_t *index, uint32_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    k_coef_unit<<<dim3((count + 255) / 256), 256, 0, s>>>(unit, stride, index, count);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_coef_unit");
    return hipGetLastError();
}

hipError_t launch_update_log(const uint8_t *coef, uint64_t stride, uint32_t rows, uint32_t count,
                             const uint16_t *log_table, uint16_t *logs, hipStream_t s) {
    if (!count || !rows) return hipSuccess;
    if (rows > 65535) return hipErrorInvalidValue;
    k_coef_log<<<dim3((count + 63) / 64, rows), 64, 0, s>>>(coef, stride, rows, count, log_table, logs);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_coef_log");
    return hipGetLastError();
}

hipError_t launch_update(const UpdateArgs &A0, hipStream_t s) {
    if (!A0.packs || !A0.count || !A0.nsel || !A0.stripes) return hipSuccess;
    if (A0.stripes > 65535) return hipErrorInvalidValue;
    UpdateArgs A = A0;
    const uint32_t threads = block_threads(A.packs), tiles = (A.packs + threads - 1) / threads;
    // rows per workgroup: more rows share one read of the deltas, fewer rows make
    // more workgroups; keep about 1024 of them where the call has that many rows
    const uint64_t units = uint64_t(A.nsel) * tiles * A.stripes;
    A.rows_per_group = uint32_t(units / 1024 < 1 ? 1 : units / 1024 > 16 ? 16 : units / 1024);
    const dim3 grid(tiles, (A.nsel + A.rows_per_group - 1) / A.rows_per_group, A.stripes);
    if (grid.y > 65535) return hipErrorInvalidValue;
    if (A.old_rows) k_update<true><<<grid, threads, 0, s>>>(A);
    else k_update<false><<<grid, threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_update<%s>", A.old_rows ? "true" : "false");
    return hipGetLastError();
}

hipError_t launch_update_lists(const UpdateListsArgs &A0, hipStream_t s) {
    if (!A0.packs || !A0.index_pitch || !A0.M || !A0.stripes) return hipSuccess;
    if (A0.stripes > 65535 || A0.M > 65536) return hipErrorInvalidValue;
    UpdateListsArgs A = A0;
    const uint32_t threads = block_threads(A.packs), tiles = (A.packs + threads - 1) / threads;
    // launch_update's rule, over every recovery row
    const uint64_t units = uint64_t(A.M) * tiles * A.stripes;
    A.rows_per_group = uint32_t(units / 1024 < 1 ? 1 : units / 1024 > 16 ? 16 : units / 1024);
    const dim3 grid(tiles, (A.M + A.rows_per_group - 1) / A.rows_per_group, A.stripes);
    if (grid.y > 65535) return hipErrorInvalidValue;
    if (A.old_rows) k_update_lists<true><<<grid, threads, 0, s>>>(A);
    else k_update_lists<false><<<grid, threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_update_lists<%s>", A.old_rows ? "true" : "false");
    return hipGetLastError();
}

hipError_t launch_update_xor(const UpdateXorArgs &A, hipStream_t s) {
    if (!A.packs || !A.nrows) return hipSuccess;
    if (A.nrows > 65535) return hipErrorInvalidValue;
    const uint32_t threads = block_threads(A.packs);
    k_rows_xor<<<dim3((A.packs + threads - 1) / threads, A.nrows), threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_rows_xor");
    return hipGetLastError();
}

}  // namespace rs
