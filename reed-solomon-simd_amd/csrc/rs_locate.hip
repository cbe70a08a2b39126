// Kernels of a locate (rs_locate_device*, DESIGN.md "Locate"): which single
// original of a stripe is corrupt?
//
// With D_j = recovery_j ^ encode(originals)_j and original i alone wrong by e (an
// element per column), D_j = G[j][i] * e in every column and for every row j
// (G: the update's coefficient matrix, rs_update.hip).  After the unfused verify
// (the encode in scratch, k_verify_rows' flags):
//
//   k_coef_unit_slab / k_coef_log_slab   the update's coefficient step over a slab
//                      of consecutive originals: the table log G[j][i], M x N
//   k_locate_find      one workgroup per stripe: CLEAN / ROWS from the flags; else
//                      the first column with D_j0 != 0, the log ratio of D_j1 and
//                      D_j0 there (j0, j1: the first two selected rows), and the i
//                      whose two table entries have that ratio
//   k_locate_confirm   D_j == (D_j0 / G[j0][i]) * G[j][i] over every selected row and
//                      pack of the stripes that name an i; a refutation stores
//                      RS_LOCATE_UNKNOWN
//   k_locate_find_masks / k_locate_confirm_masks   the two with a row list and a count
//                      per stripe (rs_locate_device_batch_masks); a
//                      stripe with fewer than two rows is skipped unread
//
// and of a heal (rs_heal_device*, DESIGN.md "Heal"), after the confirm and while
// the encode is still in scratch:
//
//   k_heal             a located original i: original_i ^= D_j0 / G[j0][i] (the
//                      confirm's e, recomputed); a ROWS stripe within the caller's
//                      threshold: its flagged selected rows copied from the scratch;
//                      one action byte per stripe
//   k_heal_masks       k_heal with a row list and a count per stripe
//                      (rs_heal_device_batch_masks), after the two
//                      *_masks kernels above; a skipped stripe costs its action byte
//
// and of a degraded locate (rs_locate_device_degraded*, DESIGN.md "Degraded locate"),
// whose `want` is the repair's second output and whose table is over information
// positions (present originals and the reference recovery rows):
//
//   k_coef_unit_degraded   the unit stripe of a slab of information positions
//   k_locate_rename        a located position that is a missing original: N + the
//                          reference row that stands in for it
//
// and of a degraded heal (rs_heal_device_degraded*, DESIGN.md "Degraded heal"), between
// the confirm and the rename of a degraded locate, while located[b] is still the
// information position q and the completed stripe's encode is still in scratch:
//
//   k_coef_log_rows        k_coef_log_slab over a row list: the table log U[r][q], m x N,
//                          from the restored rows of the unit stripe's repair
//   k_heal_degraded        a located position q: the shard it lives in ^= e (e = D_j0 /
//                          T[j0][q], the confirm's) and restored row r ^= U[r][q] * e for
//                          every missing original; a ROWS stripe: k_heal's copy of the
//                          flagged check rows; one action byte per stripe
//
// No ordering hazard inside k_heal_degraded, by construction: e comes from check row
// K[0] of the caller's recovery matrix and from scratch, and neither is ever written on
// a located stripe (the located shard is a present original or a reference row, the
// restored rows are the missing originals'); each pack of the located shard is
// read-modify-written by exactly one lane (row group 0 of its pack tile), and each pack
// of a restored row by the one lane of the one row group that owns the row (r mod the
// number of row groups), from the row itself and e alone.  Where the restored matrix
// is the originals', its rows were written by the repair earlier on the same stream.
#include <cstdio>

#include "rs_device.hpp"
#include "rs_gf.hpp"

namespace rs {
namespace {

// (rs_update.hip) a load through the constant address space from a wave-uniform
// address goes through the scalar cache into SGPRs
typedef const __attribute__((address_space(4))) uint32_t *ConstWords;
__device__ __forceinline__ ConstWords const_words(const void *p) {
    return (ConstWords)(reinterpret_cast<uintptr_t>(p));
}

constexpr int kTableWords = 20;  // words of one perm table (gf_tables.hpp kPermWords)
constexpr uint32_t kNoLog = kUpdateNoCoef;
constexpr uint32_t kFindThreads = 256;
constexpr uint32_t kFindUnroll = 4;

// Element c of the slab (original i0 + c) = 1, in the unit stripe's layout
// (rs_device.hpp launch_update_unit).
__global__ void k_coef_unit_slab(uint8_t *unit, uint64_t stride, uint32_t i0, uint32_t count) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    unit[uint64_t(i0 + c) * stride + (c >> 5) * 64u + (c & 31u)] = 1;
}

// logs[j * pitch + i0 + c] = log of element c of recovery row j; log[0] = kNoLog.
__global__ void k_coef_log_slab(const uint8_t *coef, uint64_t stride, uint32_t rows, uint32_t i0, uint32_t count,
                                uint32_t pitch, const uint16_t *log_table, uint16_t *logs) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (c >= count || j >= rows) return;
    const uint8_t *p = coef + uint64_t(j) * stride + (c >> 5) * 64u + (c & 31u);
    logs[uint64_t(j) * pitch + i0 + c] = log_table[uint32_t(p[0]) | uint32_t(p[32]) << 8];
}

// The unit stripe of a degraded locate's slab (rs_locate_device_degraded*, DESIGN.md
// "Degraded locate"): element c = 1 in the shard that information position i0 + c
// lives in -- map[p] = p: original p; N + j: recovery row j, which stands in for the
// missing original p.  The rows of both unit matrices are zeroed ahead of it.
__global__ void k_coef_unit_degraded(uint8_t *unit_orig, uint8_t *unit_rec, uint64_t stride, const int32_t *map,
                                     uint32_t N, uint32_t i0, uint32_t count) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    const uint32_t t = uint32_t(map[i0 + c]);
    uint8_t *row = t < N ? unit_orig + uint64_t(t) * stride : unit_rec + uint64_t(t - N) * stride;
    row[(c >> 5) * 64u + (c & 31u)] = 1;
}

// After the confirm of a degraded locate: a located information position that is a
// missing original becomes N + the recovery row standing in for it.  One thread per stripe.
__global__ void k_locate_rename(int32_t *located, const int32_t *map, uint32_t N, uint32_t stripes) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= stripes) return;
    const int32_t p = located[b];
    if (p >= 0 && uint32_t(p) < N) located[b] = map[p];
}

// D of pack io of row j of stripe-relative bases want / have.
__device__ __forceinline__ void ld_syndrome(const LocateArgs &A, const uint8_t *want, const uint8_t *have, uint32_t j,
                                            const PackIO &io, uint32_t &dl, uint32_t &dh) {
    const uint8_t *w = want + uint64_t(j) * A.want_stride + io.lo;
    const uint8_t *h = have + uint64_t(j) * A.have_stride + io.lo;
    dl = ld_word(w, io) ^ ld_word(h, io);
    dh = ld_word(w + io.hi_delta, io) ^ ld_word(h + io.hi_delta, io);
}

// One workgroup per stripe; every branch below is uniform over the workgroup.
__global__ __launch_bounds__(kFindThreads) void k_locate_find(const LocateArgs A) {
    __shared__ uint32_t s_count, s_pack, s_found;
    const uint32_t tid = threadIdx.x;
    const uint64_t b = blockIdx.x;
    if (tid == 0) s_count = 0, s_pack = 0xFFFFFFFFu, s_found = 0xFFFFFFFFu;
    __syncthreads();
    // unselected rows' flags are zero: the sum counts the selected rows that differ
    const uint8_t *flags = A.flags + b * A.flag_bstride;
    uint32_t c = 0;
    for (uint32_t j = tid; j < A.M; j += kFindThreads) c += flags[j] != 0;
    if (c) atomicAdd(&s_count, c);
    __syncthreads();
    const uint32_t differ = s_count;
    if (A.differ && tid == 0) A.differ[b] = differ;
    if (differ < A.nsel) {  // most stripes of a scrub end here
        if (tid == 0) A.located[b] = differ ? kLocateRows : kLocateClean;
        return;
    }
    const uint32_t j0 = A.rows ? A.rows[0] : 0u, j1 = A.rows ? A.rows[1] : 1u;
    const uint8_t *want = A.want + b * A.want_bstride, *have = A.have + b * A.have_bstride;
    // the first pack in which row j0 differs: kFindUnroll packs per thread between two barriers
    for (uint32_t base = 0; base < A.packs; base += kFindThreads * kFindUnroll) {
        uint32_t first = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t k = kFindUnroll; k-- > 0;) {
            const uint32_t pk = base + k * kFindThreads + tid;
            uint32_t dl = 0, dh = 0;
            if (pk < A.packs) ld_syndrome(A, want, have, j0, pack_io(A.fmt, pk), dl, dh);
            if (dl | dh) first = pk;
        }
        if (__syncthreads_or(first != 0xFFFFFFFFu)) {
            if (first != 0xFFFFFFFFu) atomicMin(&s_pack, first);
            break;
        }
    }
    __syncthreads();
    const uint32_t pk = s_pack;
    int32_t result = kLocateUnknown;
    if (pk < A.packs) {
        const PackIO io = pack_io(A.fmt, pk);
        uint32_t l0, h0, l1, h1;
        ld_syndrome(A, want, have, j0, io, l0, h0);
        ld_syndrome(A, want, have, j1, io, l1, h1);
        uint32_t k = 0;  // the pack's first element with D_j0 != 0
        while (k < 3 && !(((l0 | h0) >> (8 * k)) & 0xFFu)) ++k;
        const uint32_t d0 = ((l0 >> (8 * k)) & 0xFFu) | ((h0 >> (8 * k)) & 0xFFu) << 8;
        const uint32_t d1 = ((l1 >> (8 * k)) & 0xFFu) | ((h1 >> (8 * k)) & 0xFFu) << 8;
        if (d0 && d1) {  // D_j1 = 0 where D_j0 != 0: no single original (no coefficient is the sentinel's)
            const uint32_t ratio = (uint32_t(A.log_table[d1]) + 65535u - A.log_table[d0]) % 65535u;
            const uint16_t *r0 = A.logs + uint64_t(j0) * A.N, *r1 = A.logs + uint64_t(j1) * A.N;
            for (uint32_t i = tid; i < A.N; i += kFindThreads) {
                const uint32_t g0 = r0[i], g1 = r1[i];
                if (g0 != kNoLog && g1 != kNoLog && (g1 + 65535u - g0) % 65535u == ratio) atomicMin(&s_found, i);
            }
            __syncthreads();
            if (s_found < A.N) result = int32_t(s_found);
        }
    }
    if (tid == 0) A.located[b] = result;
}

// log G[j][loc] from the table, wave-uniform (j and loc are).
__device__ __forceinline__ uint32_t coef_log(ConstWords logs, uint32_t N, uint32_t j, uint32_t loc) {
    const uint32_t e = j * N + loc;
    return __builtin_amdgcn_readfirstlane((logs[e >> 1] >> ((e & 1u) * 16u)) & 0xFFFFu);
}

// e = D_j0 / G[j0][loc] of pack io (zero where !ok); the log is not the sentinel:
// k_locate_find took loc from a ratio of two logs
__device__ __forceinline__ void locate_error(const LocateArgs &A, ConstWords logs, ConstWords lut, uint32_t j0,
                                             uint32_t loc, const uint8_t *want, const uint8_t *have, const PackIO &io,
                                             bool ok, uint32_t &el, uint32_t &eh) {
    const uint32_t inv0 = (65535u - coef_log(logs, A.N, j0, loc)) % 65535u;
    uint32_t t[kTableWords], l0 = 0, h0 = 0;
#pragma unroll
    for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(inv0) * kTableWords + w];
    if (ok) ld_syndrome(A, want, have, j0, io, l0, h0);
    el = 0, eh = 0;
    gf_muladd4(el, eh, l0, h0, t);
}

// One thread per pack; blockIdx.y = group of rows_per_group selected rows,
// blockIdx.z = stripe.  The stripe's result, row numbers, logs and tables are
// wave-uniform.  Stripes without a candidate leave at once.
__global__ __launch_bounds__(256) void k_locate_confirm(const LocateArgs A) {
    const uint64_t b = blockIdx.z;
    const int32_t loc = __builtin_amdgcn_readfirstlane(A.located[b]);
    if (loc < 0) return;  // clean, ROWS, unknown, or refuted by another workgroup already
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = pk < A.packs;
    const PackIO io = pack_io(A.fmt, ok ? pk : 0u);
    const uint8_t *want = A.want + b * A.want_bstride, *have = A.have + b * A.have_bstride;
    const ConstWords logs = const_words(A.logs), lut = const_words(A.lut), rows = const_words(A.rows);
    auto log_of = [&](uint32_t j) { return coef_log(logs, A.N, j, uint32_t(loc)); };
    const uint32_t j0 = A.rows ? rows[0] : 0u;
    uint32_t el, eh;  // e = D_j0 / G[j0][i], once per workgroup
    locate_error(A, logs, lut, j0, uint32_t(loc), want, have, io, ok, el, eh);

    const uint32_t r0 = blockIdx.y * A.rows_per_group;
    const uint32_t r1 = r0 + A.rows_per_group < A.nsel ? r0 + A.rows_per_group : A.nsel;
    bool refuted = false;
    for (uint32_t r = r0 ? r0 : 1u; r < r1; ++r) {  // entry 0 is row j0 itself
        const uint32_t j = A.rows ? rows[r] : r;
        const uint32_t lg = log_of(j);
        uint32_t dl = 0, dh = 0;
        if (ok) ld_syndrome(A, want, have, j, io, dl, dh);
        // D_j against e * G[j][i]; a zero coefficient (the sentinel) makes the product zero
        uint32_t pl = 0, ph = 0;
        if (lg != kNoLog) {
            uint32_t t[kTableWords];
#pragma unroll
            for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(lg) * kTableWords + w];
            gf_muladd4(pl, ph, el, eh, t);
        }
        refuted |= pl != dl || ph != dh;
    }
    if (refuted) A.located[b] = kLocateUnknown;  // every refuting lane stores the same word
}

// k_locate_find with stripe b's own row list (rs_device.hpp LocateMaskArgs): j0, j1 and
// the count of selected rows are the stripe's.  A stripe that selects fewer than two
// rows is skipped before anything of it is read, its flags included.
__global__ __launch_bounds__(kFindThreads) void k_locate_find_masks(const LocateMaskArgs A) {
    __shared__ uint32_t s_count, s_pack, s_found;
    const uint32_t tid = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint32_t nsel = A.counts[b];
    if (nsel < 2) {
        if (tid == 0) A.located[b] = kLocateSkipped;
        return;
    }
    if (tid == 0) s_count = 0, s_pack = 0xFFFFFFFFu, s_found = 0xFFFFFFFFu;
    __syncthreads();
    const uint8_t *flags = A.flags + b * A.flag_bstride;
    uint32_t c = 0;
    for (uint32_t j = tid; j < A.M; j += kFindThreads) c += flags[j] != 0;
    if (c) atomicAdd(&s_count, c);
    __syncthreads();
    const uint32_t differ = s_count;
    if (A.differ && tid == 0) A.differ[b] = differ;
    if (differ < nsel) {
        if (tid == 0) A.located[b] = differ ? kLocateRows : kLocateClean;
        return;
    }
    const uint32_t *rows = A.rows + b * A.list_stride;
    const uint32_t j0 = rows[0], j1 = rows[1];
    const uint8_t *want = A.want + b * A.want_bstride, *have = A.have + b * A.have_bstride;
    for (uint32_t base = 0; base < A.packs; base += kFindThreads * kFindUnroll) {
        uint32_t first = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t k = kFindUnroll; k-- > 0;) {
            const uint32_t pk = base + k * kFindThreads + tid;
            uint32_t dl = 0, dh = 0;
            if (pk < A.packs) ld_syndrome(A, want, have, j0, pack_io(A.fmt, pk), dl, dh);
            if (dl | dh) first = pk;
        }
        if (__syncthreads_or(first != 0xFFFFFFFFu)) {
            if (first != 0xFFFFFFFFu) atomicMin(&s_pack, first);
            break;
        }
    }
    __syncthreads();
    const uint32_t pk = s_pack;
    int32_t result = kLocateUnknown;
    if (pk < A.packs) {
        const PackIO io = pack_io(A.fmt, pk);
        uint32_t l0, h0, l1, h1;
        ld_syndrome(A, want, have, j0, io, l0, h0);
        ld_syndrome(A, want, have, j1, io, l1, h1);
        uint32_t k = 0;
        while (k < 3 && !(((l0 | h0) >> (8 * k)) & 0xFFu)) ++k;
        const uint32_t d0 = ((l0 >> (8 * k)) & 0xFFu) | ((h0 >> (8 * k)) & 0xFFu) << 8;
        const uint32_t d1 = ((l1 >> (8 * k)) & 0xFFu) | ((h1 >> (8 * k)) & 0xFFu) << 8;
        if (d0 && d1) {
            const uint32_t ratio = (uint32_t(A.log_table[d1]) + 65535u - A.log_table[d0]) % 65535u;
            const uint16_t *r0 = A.logs + uint64_t(j0) * A.N, *r1 = A.logs + uint64_t(j1) * A.N;
            for (uint32_t i = tid; i < A.N; i += kFindThreads) {
                const uint32_t g0 = r0[i], g1 = r1[i];
                if (g0 != kNoLog && g1 != kNoLog && (g1 + 65535u - g0) % 65535u == ratio) atomicMin(&s_found, i);
            }
            __syncthreads();
            if (s_found < A.N) result = int32_t(s_found);
        }
    }
    if (tid == 0) A.located[b] = result;
}

// k_locate_confirm with stripe b's own row list and count; the grid's row groups
// cover the batch's largest count, and a group past its stripe's count has no row.
__global__ __launch_bounds__(256) void k_locate_confirm_masks(const LocateMaskArgs A) {
    const uint64_t b = blockIdx.z;
    const int32_t loc = __builtin_amdgcn_readfirstlane(A.located[b]);
    if (loc < 0) return;  // clean, ROWS, unknown, skipped, or refuted by another workgroup already
    const ConstWords logs = const_words(A.logs), lut = const_words(A.lut);
    const ConstWords rows = const_words(A.rows + b * A.list_stride);
    const uint32_t nsel = const_words(A.counts)[b];
    const uint32_t r0 = blockIdx.y * A.rows_per_group;
    const uint32_t r1 = r0 + A.rows_per_group < nsel ? r0 + A.rows_per_group : nsel;
    if ((r0 ? r0 : 1u) >= r1) return;
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = pk < A.packs;
    const PackIO io = pack_io(A.fmt, ok ? pk : 0u);
    const uint8_t *want = A.want + b * A.want_bstride, *have = A.have + b * A.have_bstride;
    uint32_t el, eh;  // e = D_j0 / G[j0][i], once per workgroup
    locate_error(A, logs, lut, rows[0], uint32_t(loc), want, have, io, ok, el, eh);
    bool refuted = false;
    for (uint32_t r = r0 ? r0 : 1u; r < r1; ++r) {  // entry 0 is row j0 itself
        const uint32_t j = rows[r];
        const uint32_t lg = coef_log(logs, A.N, j, uint32_t(loc));
        uint32_t dl = 0, dh = 0;
        if (ok) ld_syndrome(A, want, have, j, io, dl, dh);
        uint32_t pl = 0, ph = 0;
        if (lg != kNoLog) {
            uint32_t t[kTableWords];
#pragma unroll
            for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(lg) * kTableWords + w];
            gf_muladd4(pl, ph, el, eh, t);
        }
        refuted |= pl != dl || ph != dh;
    }
    if (refuted) A.located[b] = kLocateUnknown;  // every refuting lane stores the same word
}

// The confirm's grid.  Every branch but the pack bound is uniform over the
// workgroup; a stripe with nothing to heal (the common one of a scrub) leaves at once.
__global__ __launch_bounds__(256) void k_heal(const HealArgs A) {
    const uint64_t b = blockIdx.z;
    const int32_t loc = __builtin_amdgcn_readfirstlane(A.located[b]);
    uint32_t action = 0;
    if (loc >= 0) {
        if (A.mode & kHealOriginal) action = kHealOriginal;
    } else if (loc == kLocateRows && (A.mode & kHealRecovery)) {
        if (uint32_t(__builtin_amdgcn_readfirstlane(A.differ[b])) <= A.max_rows) action = kHealRecovery;
    }
    if ((blockIdx.x | blockIdx.y | threadIdx.x) == 0) A.action[b] = uint8_t(action);
    if (!action) return;
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = pk < A.packs;
    const PackIO io = pack_io(A.fmt, ok ? pk : 0u);
    const uint8_t *want = A.want + b * A.want_bstride;
    const ConstWords rows = const_words(A.rows);
    if (action == kHealOriginal) {
        if (blockIdx.y) return;  // one row to write: row group 0 does it
        uint32_t el, eh;
        locate_error(A, const_words(A.logs), const_words(A.lut), A.rows ? rows[0] : 0u, uint32_t(loc), want,
                     A.have + b * A.have_bstride, io, ok, el, eh);
        if (!ok) return;
        uint8_t *p = A.orig + b * A.orig_bstride + uint64_t(loc) * A.orig_stride + io.lo;
        st_word(p, ld_word(p, io) ^ el, io);
        st_word(p + io.hi_delta, ld_word(p + io.hi_delta, io) ^ eh, io);
        return;
    }
    const uint8_t *flags = A.flags + b * A.flag_bstride;
    uint8_t *rec = A.rec + b * A.have_bstride;
    const uint32_t r0 = blockIdx.y * A.rows_per_group;
    const uint32_t r1 = r0 + A.rows_per_group < A.nsel ? r0 + A.rows_per_group : A.nsel;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t j = A.rows ? rows[r] : r;
        if (!__builtin_amdgcn_readfirstlane(uint32_t(flags[j])) || !ok) continue;
        const uint8_t *w = want + uint64_t(j) * A.want_stride + io.lo;
        uint8_t *h = rec + uint64_t(j) * A.have_stride + io.lo;
        st_word(h, ld_word(w, io), io);
        st_word(h + io.hi_delta, ld_word(w + io.hi_delta, io), io);
    }
}

// k_heal with stripe b's own row list and count (rs_device.hpp HealMaskArgs), on the grid
// of k_locate_confirm_masks: j0 is the STRIPE's first selected row, and a row group at or
// past the stripe's count has no row.  A skipped stripe (located[b] = kLocateSkipped)
// costs its action byte and nothing else: its flags, differ[b], rows and matrices are
// never read.
__global__ __launch_bounds__(256) void k_heal_masks(const HealMaskArgs A) {
    const uint64_t b = blockIdx.z;
    const int32_t loc = __builtin_amdgcn_readfirstlane(A.located[b]);
    uint32_t action = 0;
    if (loc >= 0) {
        if (A.mode & kHealOriginal) action = kHealOriginal;
    } else if (loc == kLocateRows && (A.mode & kHealRecovery)) {
        if (uint32_t(__builtin_amdgcn_readfirstlane(A.differ[b])) <= A.max_rows) action = kHealRecovery;
    }
    if ((blockIdx.x | blockIdx.y | threadIdx.x) == 0) A.action[b] = uint8_t(action);
    if (!action) return;
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = pk < A.packs;
    const PackIO io = pack_io(A.fmt, ok ? pk : 0u);
    const uint8_t *want = A.want + b * A.want_bstride;
    const ConstWords rows = const_words(A.rows + b * A.list_stride);
    if (action == kHealOriginal) {
        if (blockIdx.y) return;  // one row to write: row group 0 does it
        uint32_t el, eh;
        locate_error(A, const_words(A.logs), const_words(A.lut), rows[0], uint32_t(loc), want,
                     A.have + b * A.have_bstride, io, ok, el, eh);
        if (!ok) return;
        uint8_t *p = A.orig + b * A.orig_bstride + uint64_t(loc) * A.orig_stride + io.lo;
        st_word(p, ld_word(p, io) ^ el, io);
        st_word(p + io.hi_delta, ld_word(p + io.hi_delta, io) ^ eh, io);
        return;
    }
    const uint32_t nsel = const_words(A.counts)[b];
    const uint32_t r0 = blockIdx.y * A.rows_per_group;
    const uint32_t r1 = r0 + A.rows_per_group < nsel ? r0 + A.rows_per_group : nsel;
    if (r0 >= r1) return;
    const uint8_t *flags = A.flags + b * A.flag_bstride;
    uint8_t *rec = A.rec + b * A.have_bstride;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t j = rows[r];
        if (!__builtin_amdgcn_readfirstlane(uint32_t(flags[j])) || !ok) continue;
        const uint8_t *w = want + uint64_t(j) * A.want_stride + io.lo;
        uint8_t *h = rec + uint64_t(j) * A.have_stride + io.lo;
        st_word(h, ld_word(w, io), io);
        st_word(h + io.hi_delta, ld_word(w + io.hi_delta, io), io);
    }
}

// k_coef_log_slab over the rows a list names: logs[r * pitch + i0 + c] = log of element
// c of row rows[r] of `coef`, r < nrows (a degraded heal's table log U: coef is the
// first output of the unit stripe's repair, rows the missing originals).
__global__ void k_coef_log_rows(const uint8_t *coef, uint64_t stride, const uint32_t *rows, uint32_t nrows, uint32_t i0,
                                uint32_t count, uint32_t pitch, const uint16_t *log_table, uint16_t *logs) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (c >= count || r >= nrows) return;
    const uint8_t *p = coef + uint64_t(rows[r]) * stride + (c >> 5) * 64u + (c & 31u);
    logs[uint64_t(r) * pitch + i0 + c] = log_table[uint32_t(p[0]) | uint32_t(p[32]) << 8];
}

// The confirm's x and z; gridDim.y = the row groups of rows_per_group rows over max(m,
// nsel) rows.  On a ROWS stripe group y has check rows y * rows_per_group ...; on a
// located stripe the m restored rows are dealt round the groups (row r to group r mod
// gridDim.y), so that few missing originals under many check rows still spread over m
// workgroups per pack tile.  The grid is sized for the ROWS case on purpose: on a
// located stripe only the groups y < m have a row, each of them forms e for itself (one
// syndrome load of row K[0] and one table fetch), and the others leave after two scalar
// loads.  located[b] is still an information position.  Every branch
// but the pack bound is uniform over the workgroup; workgroup (0, 0) of a stripe stores
// action[b]; a stripe with nothing to heal leaves at once, and so does a row group with
// no row.
__global__ __launch_bounds__(256) void k_heal_degraded(const HealDegradedArgs A) {
    const uint64_t b = blockIdx.z;
    const int32_t loc = __builtin_amdgcn_readfirstlane(A.located[b]);
    uint32_t action = 0, shard = 0;
    if (loc >= 0) {  // the shard position loc lives in: original loc, or N + a reference row
        shard = __builtin_amdgcn_readfirstlane(const_words(A.map)[loc]);
        const uint32_t bit = shard < A.N ? kHealOriginal : kHealRecovery;
        if (A.mode & bit) action = bit;
    } else if (loc == kLocateRows && (A.mode & kHealRecovery)) {
        if (uint32_t(__builtin_amdgcn_readfirstlane(A.differ[b])) <= A.max_rows) action = kHealRecovery;
    }
    if ((blockIdx.x | blockIdx.y | threadIdx.x) == 0) A.action[b] = uint8_t(action);
    if (!action) return;
    const uint32_t r0 = blockIdx.y * A.rows_per_group;
    const uint32_t r1 = r0 + A.rows_per_group < A.nsel ? r0 + A.rows_per_group : A.nsel;
    if (loc >= 0 ? blockIdx.y >= A.m : r0 >= A.nsel) return;  // (row group 0 always has a row: m >= 1, nsel >= 2)
    const uint32_t pk = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = pk < A.packs;
    const PackIO io = pack_io(A.fmt, ok ? pk : 0u);
    const uint8_t *want = A.want + b * A.want_bstride;
    const ConstWords rows = const_words(A.rows);
    if (loc >= 0) {
        const ConstWords lut = const_words(A.lut), logu = const_words(A.logu), miss = const_words(A.miss);
        uint32_t el, eh;  // e = D_j0 / T[j0][loc], once per workgroup
        locate_error(A, const_words(A.logs), lut, rows[0], uint32_t(loc), want, A.have + b * A.have_bstride, io, ok, el,
                     eh);
        if (blockIdx.y == 0 && ok) {
            uint8_t *p = shard < A.N ? A.orig + b * A.orig_bstride + uint64_t(shard) * A.orig_stride
                                     : A.rec + b * A.have_bstride + uint64_t(shard - A.N) * A.have_stride;
            p += io.lo;
            st_word(p, ld_word(p, io) ^ el, io);
            st_word(p + io.hi_delta, ld_word(p + io.hi_delta, io) ^ eh, io);
        }
        uint8_t *out = A.restored + b * A.restored_bstride;
        for (uint32_t r = blockIdx.y; r < A.m; r += gridDim.y) {
            // restored row r ^= U[r][loc] * e (no entry of U is zero; the sentinel would add nothing)
            const uint32_t lg = coef_log(logu, A.N, r, uint32_t(loc));
            uint32_t pl = 0, ph = 0;
            if (lg != kNoLog) {
                uint32_t t[kTableWords];
#pragma unroll
                for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(lg) * kTableWords + w];
                gf_muladd4(pl, ph, el, eh, t);
            }
            if (!ok) continue;
            uint8_t *p = out + uint64_t(miss[r]) * A.restored_stride + io.lo;
            st_word(p, ld_word(p, io) ^ pl, io);
            st_word(p + io.hi_delta, ld_word(p + io.hi_delta, io) ^ ph, io);
        }
        return;
    }
    // a ROWS stripe within the threshold: k_heal's copy of the flagged check rows
    const uint8_t *flags = A.flags + b * A.flag_bstride;
    uint8_t *rec = A.rec + b * A.have_bstride;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t j = rows[r];
        if (!__builtin_amdgcn_readfirstlane(uint32_t(flags[j])) || !ok) continue;
        const uint8_t *w = want + uint64_t(j) * A.want_stride + io.lo;
        uint8_t *h = rec + uint64_t(j) * A.have_stride + io.lo;
        st_word(h, ld_word(w, io), io);
        st_word(h + io.hi_delta, ld_word(w + io.hi_delta, io), io);
    }
}

}  // namespace

hipError_t launch_locate_unit(uint8_t *unit, uint64_t stride, uint32_t i0, uint32_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    k_coef_unit_slab<<<dim3((count + 255) / 256), 256, 0, s>>>(unit, stride, i0, count);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_coef_unit_slab");
    return hipGetLastError();
}

hipError_t launch_locate_unit_degraded(uint8_t *unit_orig, uint8_t *unit_rec, uint64_t stride, const int32_t *map,
                                       uint32_t N, uint32_t i0, uint32_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    if (!map || uint64_t(i0) + count > N || stride < 64 * ((uint64_t(count) + 31) / 32)) return hipErrorInvalidValue;
    k_coef_unit_degraded<<<dim3((count + 255) / 256), 256, 0, s>>>(unit_orig, unit_rec, stride, map, N, i0, count);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_coef_unit_degraded");
    return hipGetLastError();
}

hipError_t launch_locate_rename(int32_t *located, const int32_t *map, uint32_t N, uint32_t stripes, hipStream_t s) {
    if (!stripes) return hipSuccess;
    if (!located || !map) return hipErrorInvalidValue;
    k_locate_rename<<<dim3((stripes + 255) / 256), 256, 0, s>>>(located, map, N, stripes);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_locate_rename");
    return hipGetLastError();
}

hipError_t launch_locate_log(const uint8_t *coef, uint64_t stride, uint32_t rows, uint32_t i0, uint32_t count,
                             uint32_t pitch, const uint16_t *log_table, uint16_t *logs, hipStream_t s) {
    if (!count || !rows) return hipSuccess;
    if (rows > 65535 || uint64_t(i0) + count > pitch) return hipErrorInvalidValue;
    k_coef_log_slab<<<dim3((count + 63) / 64, rows), 64, 0, s>>>(coef, stride, rows, i0, count, pitch, log_table, logs);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_coef_log_slab");
    return hipGetLastError();
}

hipError_t launch_locate_find(const LocateArgs &A, hipStream_t s) {
    if (!A.stripes) return hipSuccess;
    if (A.nsel < 2 || A.nsel > A.M || !A.packs || !A.N) return hipErrorInvalidValue;
    k_locate_find<<<dim3(A.stripes), kFindThreads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_locate_find");
    return hipGetLastError();
}

hipError_t launch_locate_confirm(const LocateArgs &A0, hipStream_t s) {
    if (!A0.stripes) return hipSuccess;
    if (A0.nsel < 2 || !A0.packs || A0.stripes > 65535) return hipErrorInvalidValue;
    LocateArgs A = A0;
    const uint32_t threads = A.packs >= 256 ? 256u : (A.packs + 63u) / 64u * 64u, tiles = (A.packs + threads - 1) / threads;
    // as launch_update: about 1024 workgroups where the call has that many rows,
    // so that the stripes without a candidate cost few of them
    const uint64_t units = uint64_t(A.nsel) * tiles * A.stripes;
    A.rows_per_group = uint32_t(units / 1024 < 1 ? 1 : units / 1024 > 16 ? 16 : units / 1024);
    const dim3 grid(tiles, (A.nsel + A.rows_per_group - 1) / A.rows_per_group, A.stripes);
    if (grid.y > 65535) return hipErrorInvalidValue;
    k_locate_confirm<<<grid, threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_locate_confirm");
    return hipGetLastError();
}

hipError_t launch_locate_find_masks(const LocateMaskArgs &A, hipStream_t s) {
    if (!A.stripes) return hipSuccess;
    if (!A.rows || !A.counts || A.nsel > A.M || !A.packs || !A.N) return hipErrorInvalidValue;
    k_locate_find_masks<<<dim3(A.stripes), kFindThreads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_locate_find_masks");
    return hipGetLastError();
}

hipError_t launch_locate_confirm_masks(const LocateMaskArgs &A0, hipStream_t s) {
    if (!A0.stripes) return hipSuccess;
    if (!A0.rows || !A0.counts || A0.nsel < 2 || !A0.packs || A0.stripes > 65535) return hipErrorInvalidValue;
    LocateMaskArgs A = A0;
    // the confirm's grid (launch_locate_confirm) over the largest count
    const uint32_t threads = A.packs >= 256 ? 256u : (A.packs + 63u) / 64u * 64u, tiles = (A.packs + threads - 1) / threads;
    const uint64_t units = uint64_t(A.nsel) * tiles * A.stripes;
    A.rows_per_group = uint32_t(units / 1024 < 1 ? 1 : units / 1024 > 16 ? 16 : units / 1024);
    const dim3 grid(tiles, (A.nsel + A.rows_per_group - 1) / A.rows_per_group, A.stripes);
    if (grid.y > 65535) return hipErrorInvalidValue;
    k_locate_confirm_masks<<<grid, threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_locate_confirm_masks");
    return hipGetLastError();
}

hipError_t launch_heal(const HealArgs &A0, hipStream_t s) {
    if (!A0.stripes) return hipSuccess;
    if (A0.nsel < 2 || !A0.packs || A0.stripes > 65535 || !A0.differ || !A0.action || !A0.orig || !A0.rec ||
        !A0.mode || (A0.mode & ~(kHealOriginal | kHealRecovery)))
        return hipErrorInvalidValue;
    HealArgs A = A0;
    // the confirm's grid (launch_locate_confirm)
    const uint32_t threads = A.packs >= 256 ? 256u : (A.packs + 63u) / 64u * 64u, tiles = (A.packs + threads - 1) / threads;
    const uint64_t units = uint64_t(A.nsel) * tiles * A.stripes;
    A.rows_per_group = uint32_t(units / 1024 < 1 ? 1 : units / 1024 > 16 ? 16 : units / 1024);
    const dim3 grid(tiles, (A.nsel + A.rows_per_group - 1) / A.rows_per_group, A.stripes);
    if (grid.y > 65535) return hipErrorInvalidValue;
    k_heal<<<grid, threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_heal");
    return hipGetLastError();
}

hipError_t launch_heal_masks(const HealMaskArgs &A0, hipStream_t s) {
    if (!A0.stripes) return hipSuccess;
    if (!A0.rows || !A0.counts || A0.nsel < 2 || !A0.packs || A0.stripes > 65535 || !A0.differ || !A0.action ||
        !A0.orig || !A0.rec || !A0.mode || (A0.mode & ~(kHealOriginal | kHealRecovery)))
        return hipErrorInvalidValue;
    HealMaskArgs A = A0;
    // the confirm's grid (launch_locate_confirm_masks) over the largest count
    const uint32_t threads = A.packs >= 256 ? 256u : (A.packs + 63u) / 64u * 64u, tiles = (A.packs + threads - 1) / threads;
    const uint64_t units = uint64_t(A.nsel) * tiles * A.stripes;
    A.rows_per_group = uint32_t(units / 1024 < 1 ? 1 : units / 1024 > 16 ? 16 : units / 1024);
    const dim3 grid(tiles, (A.nsel + A.rows_per_group - 1) / A.rows_per_group, A.stripes);
    if (grid.y > 65535) return hipErrorInvalidValue;
    k_heal_masks<<<grid, threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_heal_masks");
    return hipGetLastError();
}

hipError_t launch_locate_log_rows(const uint8_t *coef, uint64_t stride, const uint32_t *rows, uint32_t nrows,
                                  uint32_t i0, uint32_t count, uint32_t pitch, const uint16_t *log_table,
                                  uint16_t *logs, hipStream_t s) {
    if (!count || !nrows) return hipSuccess;
    if (!rows || nrows > 65535 || uint64_t(i0) + count > pitch || stride < 64 * ((uint64_t(count) + 31) / 32))
        return hipErrorInvalidValue;
    k_coef_log_rows<<<dim3((count + 63) / 64, nrows), 64, 0, s>>>(coef, stride, rows, nrows, i0, count, pitch,
                                                                   log_table, logs);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_coef_log_rows");
    return hipGetLastError();
}

hipError_t launch_heal_degraded(const HealDegradedArgs &A0, hipStream_t s) {
    if (!A0.stripes) return hipSuccess;
    if (A0.nsel < 2 || !A0.packs || A0.stripes > 65535 || !A0.rows || !A0.differ || !A0.action || !A0.orig ||
        !A0.rec || !A0.mode || (A0.mode & ~(kHealOriginal | kHealRecovery)) || !A0.m || A0.m > A0.N || !A0.map ||
        !A0.miss || !A0.logu || !A0.restored)
        return hipErrorInvalidValue;
    HealDegradedArgs A = A0;
    // the confirm's x and z (launch_locate_confirm); y over the larger of the two row counts
    const uint32_t threads = A.packs >= 256 ? 256u : (A.packs + 63u) / 64u * 64u, tiles = (A.packs + threads - 1) / threads;
    const uint32_t nrows = A.m > A.nsel ? A.m : A.nsel;
    const uint64_t units = uint64_t(nrows) * tiles * A.stripes;
    A.rows_per_group = uint32_t(units / 1024 < 1 ? 1 : units / 1024 > 16 ? 16 : units / 1024);
    const dim3 grid(tiles, (nrows + A.rows_per_group - 1) / A.rows_per_group, A.stripes);
    if (grid.y > 65535) return hipErrorInvalidValue;
    k_heal_degraded<<<grid, threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_heal_degraded");
    return hipGetLastError();
}

}  // namespace rs
