// Kernels of a robust locate (rs_locate_device_robust*, DESIGN.md "Robust locate"):
// which single original of a stripe is corrupt, when up to t = max_outliers of the
// selected recovery rows are corrupt as well?
//
// With D_j = recovery_j ^ encode(originals)_j, original i wrong by e (an element per
// column) and a set B of at most t corrupt selected rows, D_j = G[j][i] * e in every
// column for every selected row j outside B (rs_locate.hip has the plain form, B
// empty).  Of the first t + 1 disjoint pairs of the selected-row list one at least
// has both rows outside B.  After the unfused verify (the encode in scratch,
// k_verify_rows' flags), with the locate's table log G[j][i]:
//
//   k_locate_find_pairs  one workgroup per stripe and pair: CLEAN / ROWS from the flags;
//                        else for its pair p what k_locate_find does for its two rows (the
//                        first column with D_sel[2p] != 0, the log ratio against
//                        D_sel[2p+1] there, the i whose two table entries have that
//                        ratio): candidate p = (i_p, reference row sel[2p]) or none
//   k_locate_count       the confirm's grid: every selected row's D_j, loaded once,
//                        against (D_ref / G[ref][i_p]) * G[j][i_p] of every candidate;
//                        a disagreeing lane stores the byte 1 to votes[stripe][p][j]
//   k_locate_decide      one workgroup per stripe: the first candidate with at most t
//                        bytes set gives located[b] and its bytes the stripe's
//                        outlier row; none: RS_LOCATE_UNKNOWN
//
//
// A robust heal (rs_heal_device_robust*, DESIGN.md "Robust heal") adds one launch
// after k_locate_decide, while the encode is still in scratch:
//
//   k_heal_robust        the confirm's grid.  A located stripe (i, B): e = D_r / G[r][i]
//                        from the first selected row r outside B; row group 0 writes
//                        original_i ^= e, and every row group writes its rows j of B as
//                        want_j ^ G[j][i] * e (the encode's linearity: that is the
//                        encode of the originals with e taken off original i).  A ROWS
//                        stripe: k_heal's copy of the flagged rows from the encode,
//                        when at most max_rows differ
//
// No ordering hazard inside k_heal_robust, by construction: e comes from row r of the
// caller's recovery matrix and from scratch, and neither is ever written (r is outside
// B, and only rows of B are stored to on a located stripe); each pack of original i is
// read-modify-written by exactly one lane (row group 0 of its pack tile); each outlier
// row is written by the one workgroup per pack tile that owns it, from scratch and e
// alone; a ROWS stripe's rows are copied from scratch.  The caller's matrices must not
// overlap one another or the four outputs.
//
// ConstWords, ld_syndrome and coef_log are rs_locate.hip's (copied: that file's
// kernels are not to move).
#include <cstdio>

#include "rs_device.hpp"
#include "rs_gf.hpp"

namespace rs {
namespace {

typedef const __attribute__((address_space(4))) uint32_t *ConstWords;
__device__ __forceinline__ ConstWords const_words(const void *p) {
    return (ConstWords)(reinterpret_cast<uintptr_t>(p));
}

constexpr int kTableWords = 20;  // words of one perm table (gf_tables.hpp kPermWords)
constexpr uint32_t kNoLog = kUpdateNoCoef;
constexpr uint32_t kFindThreads = 256;
constexpr uint32_t kFindUnroll = 4;
constexpr uint32_t kCands = kRobustMaxOutliers + 1;  // candidates of a stripe at most

// D of pack io of row j of stripe-relative bases want / have.
__device__ __forceinline__ void ld_syndrome(const LocateArgs &A, const uint8_t *want, const uint8_t *have, uint32_t j,
                                            const PackIO &io, uint32_t &dl, uint32_t &dh) {
    const uint8_t *w = want + uint64_t(j) * A.want_stride + io.lo;
    const uint8_t *h = have + uint64_t(j) * A.have_stride + io.lo;
    dl = ld_word(w, io) ^ ld_word(h, io);
    dh = ld_word(w + io.hi_delta, io) ^ ld_word(h + io.hi_delta, io);
}

// log G[j][loc] from the table, wave-uniform (j and loc are).
__device__ __forceinline__ uint32_t coef_log(ConstWords logs, uint32_t N, uint32_t j, uint32_t loc) {
    const uint32_t e = j * N + loc;
    return __builtin_amdgcn_readfirstlane((logs[e >> 1] >> ((e & 1u) * 16u)) & 0xFFFFu);
}

// One workgroup per stripe and pair (blockIdx.y = p <= t), so that the pairs' dependent
// loads run side by side; every branch below is uniform over the workgroup.  Each
// workgroup sums the stripe's flags for itself and writes cand[b][p]; pair 0's also
// writes located[b]: CLEAN, ROWS, or UNKNOWN until k_locate_decide has spoken.
__global__ __launch_bounds__(kFindThreads) void k_locate_find_pairs(const RobustArgs A) {
    __shared__ uint32_t s_count, s_pack, s_found;
    const uint32_t tid = threadIdx.x, p = blockIdx.y;
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
    int32_t *cand = A.cand + b * kCands;
    if (differ < A.nsel) {  // most stripes of a scrub end here
        if (tid == 0) {
            if (p == 0) A.located[b] = differ ? kLocateRows : kLocateClean;
            cand[p] = -1;
        }
        return;
    }
    if (tid == 0 && p == 0) A.located[b] = kLocateUnknown;
    const uint32_t j0 = A.rows ? A.rows[2 * p] : 2 * p, j1 = A.rows ? A.rows[2 * p + 1] : 2 * p + 1;
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
    int32_t result = -1;
    if (pk < A.packs) {
        const PackIO io = pack_io(A.fmt, pk);
        uint32_t l0, h0, l1, h1;
        ld_syndrome(A, want, have, j0, io, l0, h0);
        ld_syndrome(A, want, have, j1, io, l1, h1);
        uint32_t k = 0;  // the pack's first element with D_j0 != 0
        while (k < 3 && !(((l0 | h0) >> (8 * k)) & 0xFFu)) ++k;
        const uint32_t d0 = ((l0 >> (8 * k)) & 0xFFu) | ((h0 >> (8 * k)) & 0xFFu) << 8;
        const uint32_t d1 = ((l1 >> (8 * k)) & 0xFFu) | ((h1 >> (8 * k)) & 0xFFu) << 8;
        if (d0 && d1) {  // D_j1 = 0 where D_j0 != 0: this pair names no original
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
    if (tid == 0) cand[p] = result;
}

// One thread per pack; blockIdx.y = group of rows_per_group selected rows,
// blockIdx.z = stripe.  The stripe's candidates, row numbers, logs and tables are
// wave-uniform.  Stripes without a candidate leave at once.  A lane keeps its e of
// every candidate in LDS (slots of its own: no barrier), the candidates' originals
// and aliases packed in scalar registers, so that the loops over the candidates
// need no unrolling and no indexed registers.
__global__ __launch_bounds__(256) void k_locate_count(const RobustArgs A) {
    __shared__ uint32_t s_el[kCands][256], s_eh[kCands][256];
    const uint64_t b = blockIdx.z;
    const uint32_t tid = threadIdx.x;
    const ConstWords logs = const_words(A.logs), lut = const_words(A.lut), rows = const_words(A.rows);
    const int32_t *cand = A.cand + b * kCands;
    constexpr uint32_t kNone = 0xFFFFu;  // (an original is below 4096)
    uint64_t locs[2] = {~0ull, ~0ull};   // candidate q's original: 16 bits at 16 * (q % 4) of word q / 4
#pragma unroll
    for (uint32_t q = 0; q < kCands; ++q) {
        const int32_t l = q <= A.t ? __builtin_amdgcn_readfirstlane(cand[q]) : -1;
        if (l >= 0) locs[q >> 2] ^= uint64_t(uint32_t(l) ^ kNone) << (16 * (q & 3));
    }
    if ((locs[0] & locs[1]) == ~0ull) return;  // clean, ROWS, or no pair named an original
    const uint64_t loc_lo = locs[0], loc_hi = locs[1];
    auto loc_of = [&](uint32_t q) { return uint32_t((q < 4 ? loc_lo : loc_hi) >> (16 * (q & 3))) & kNone; };
    const uint32_t pk = blockIdx.x * blockDim.x + tid;
    const bool ok = pk < A.packs;
    const PackIO io = pack_io(A.fmt, ok ? pk : 0u);
    const uint8_t *want = A.want + b * A.want_bstride, *have = A.have + b * A.have_bstride;

    // e_q = D_ref / G[ref][i_q] with ref = sel[2q], candidate q's own reference row (the
    // log is not the sentinel: the find took i_q from a ratio of two logs).  alias, 4
    // bits per candidate: the first candidate with that i and, over this wave, that e
    // -- its verdict is q's
    uint32_t alias = 0;
    for (uint32_t q = 0; q <= A.t; ++q) {
        const uint32_t loc = loc_of(q);
        if (loc == kNone) continue;
        const uint32_t ref = A.rows ? rows[2 * q] : 2 * q;
        const uint32_t inv = (65535u - coef_log(logs, A.N, ref, loc)) % 65535u;
        uint32_t t[kTableWords], l0 = 0, h0 = 0, el = 0, eh = 0;
#pragma unroll
        for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(inv) * kTableWords + w];
        if (ok) ld_syndrome(A, want, have, ref, io, l0, h0);
        gf_muladd4(el, eh, l0, h0, t);
        s_el[q][tid] = el, s_eh[q][tid] = eh;
        uint32_t first = q;
        for (uint32_t p = q; p-- > 0;)
            if (loc_of(p) == loc && !__builtin_amdgcn_ballot_w64(s_el[p][tid] != el || s_eh[p][tid] != eh)) first = p;
        alias |= first << (4 * q);
    }

    uint8_t *votes = A.votes + b * A.vote_bstride;
    const uint32_t r0 = blockIdx.y * A.rows_per_group;
    const uint32_t r1 = r0 + A.rows_per_group < A.nsel ? r0 + A.rows_per_group : A.nsel;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t j = A.rows ? rows[r] : r;
        uint32_t dl = 0, dh = 0;
        if (ok) ld_syndrome(A, want, have, j, io, dl, dh);
        uint32_t wrong = 0;  // bit q: this lane's pack of row j disagrees with candidate q
        for (uint32_t q = 0; q <= A.t; ++q) {
            const uint32_t loc = loc_of(q), first = (alias >> (4 * q)) & 15u;
            if (loc == kNone) continue;
            if (first != q) {
                wrong |= ((wrong >> first) & 1u) << q;
                continue;
            }
            // D_j against e_q * G[j][i_q]; a zero coefficient (the sentinel) makes the product zero
            const uint32_t lg = coef_log(logs, A.N, j, loc);
            uint32_t pl = 0, ph = 0;
            if (lg != kNoLog) {
                uint32_t t[kTableWords];
#pragma unroll
                for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(lg) * kTableWords + w];
                gf_muladd4(pl, ph, s_el[q][tid], s_eh[q][tid], t);
            }
            wrong |= uint32_t(pl != dl || ph != dh) << q;
        }
        for (uint32_t q = 0; wrong >> q; ++q)
            if ((wrong >> q) & 1u) votes[uint64_t(q) * A.M + j] = 1;  // every disagreeing lane stores the same byte
    }
}

// One workgroup per stripe, after k_locate_count; every branch is uniform over it.
__global__ __launch_bounds__(kFindThreads) void k_locate_decide(const RobustArgs A) {
    __shared__ uint32_t s_count[kCands];
    const uint32_t tid = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const int32_t *cand = A.cand + b * kCands;
    const uint8_t *votes = A.votes + b * A.vote_bstride;
    if (tid < kCands) s_count[tid] = 0;
    __syncthreads();
    for (uint32_t p = 0; p <= A.t; ++p) {
        const int32_t loc = cand[p];
        if (loc < 0) continue;
        // unselected rows' bytes are zero: the sum counts the selected rows that disagree
        const uint8_t *v = votes + uint64_t(p) * A.M;
        uint32_t c = 0;
        for (uint32_t j = tid; j < A.M; j += kFindThreads) c += v[j] != 0;
        if (c) atomicAdd(&s_count[p], c);
        __syncthreads();
        if (s_count[p] > A.t) continue;
        uint8_t *out = A.outlier + b * A.outlier_bstride;  // zeroed ahead of the launch
        for (uint32_t j = tid; j < A.M; j += kFindThreads)
            if (v[j]) out[j] = 1;
        if (tid == 0) A.located[b] = loc;
        return;
    }
    // CLEAN, ROWS or UNKNOWN, as k_locate_find_pairs left it
}

// The confirm's grid, after k_locate_decide.  Every branch but the pack bound is uniform
// over the workgroup; workgroup (0, 0) of a stripe stores action[b]; a stripe with
// nothing to heal (the common one of a scrub) leaves at once, and so does a row
// group with no row to write.
__global__ __launch_bounds__(256) void k_heal_robust(const HealRobustArgs A) {
    __shared__ uint32_t s_count;
    const uint64_t b = blockIdx.z;
    const uint32_t tid = threadIdx.x;
    const int32_t loc = __builtin_amdgcn_readfirstlane(A.located[b]);
    const bool first = (blockIdx.x | blockIdx.y) == 0;
    const bool rec_bit = (A.mode & kHealRecovery) != 0;
    if (loc < 0 && !(loc == kLocateRows && rec_bit)) {  // CLEAN, UNKNOWN, or ROWS with its bit off
        if (first && tid == 0) A.action[b] = 0;
        return;
    }
    const ConstWords rows = const_words(A.rows);
    // what names the rows to write: the outlier bytes of a located stripe, the flags of a ROWS one
    const uint8_t *marks = loc >= 0 ? A.outlier + b * A.outlier_bstride : A.flags + b * A.flag_bstride;
    const uint32_t r0 = blockIdx.y * A.rows_per_group;  // (rows_per_group <= 16)
    const uint32_t r1 = r0 + A.rows_per_group < A.nsel ? r0 + A.rows_per_group : A.nsel;
    uint32_t mine = 0;  // bit r - r0: this group's selected row r is marked
    if (rec_bit)
        for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t j = A.rows ? rows[r] : r;
            mine |= uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(marks[j])) != 0) << (r - r0);
        }
    const uint32_t pk = blockIdx.x * blockDim.x + tid;
    const bool ok = pk < A.packs;
    const PackIO io = pack_io(A.fmt, ok ? pk : 0u);
    const uint8_t *want = A.want + b * A.want_bstride;
    uint8_t *rec = A.rec + b * A.have_bstride;

    if (loc >= 0) {
        const bool write_orig = (A.mode & kHealOriginal) && blockIdx.y == 0;
        if (first) {
            uint32_t action = A.mode & kHealOriginal;
            if (rec_bit) {  // B is not empty?  (unselected rows' bytes are zero)
                uint32_t c = 0;
                for (uint32_t j = tid; j < A.M; j += blockDim.x) c |= marks[j];
                if (__syncthreads_or(int(c))) action |= kHealRecovery;
            }
            if (tid == 0) A.action[b] = uint8_t(action);
        }
        if (!write_orig && !mine) return;
        // r: one of the first t + 1 selected rows is outside B
        uint32_t ref = 0;
        for (uint32_t q = 0; q <= A.t; ++q) {
            ref = A.rows ? rows[q] : q;
            if (!__builtin_amdgcn_readfirstlane(uint32_t(marks[ref]))) break;
        }
        // e = D_r / G[r][i], once per workgroup (the log is not the sentinel: row r differs and agrees)
        const ConstWords logs = const_words(A.logs), lut = const_words(A.lut);
        const uint32_t inv = (65535u - coef_log(logs, A.N, ref, uint32_t(loc))) % 65535u;
        uint32_t t[kTableWords], l0 = 0, h0 = 0, el = 0, eh = 0;
#pragma unroll
        for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(inv) * kTableWords + w];
        if (ok) ld_syndrome(A, want, A.have + b * A.have_bstride, ref, io, l0, h0);
        gf_muladd4(el, eh, l0, h0, t);
        if (write_orig && ok) {
            uint8_t *p = A.orig + b * A.orig_bstride + uint64_t(loc) * A.orig_stride + io.lo;
            st_word(p, ld_word(p, io) ^ el, io);
            st_word(p + io.hi_delta, ld_word(p + io.hi_delta, io) ^ eh, io);
        }
        for (uint32_t r = r0; mine >> (r - r0); ++r) {
            if (!((mine >> (r - r0)) & 1u)) continue;
            const uint32_t j = A.rows ? rows[r] : r;
            // want_j ^ G[j][i] * e; a zero coefficient (the sentinel) contributes nothing
            const uint32_t lg = coef_log(logs, A.N, j, uint32_t(loc));
            uint32_t pl = 0, ph = 0;
            if (lg != kNoLog) {
#pragma unroll
                for (int w = 0; w < kTableWords; ++w) t[w] = lut[uint64_t(lg) * kTableWords + w];
                gf_muladd4(pl, ph, el, eh, t);
            }
            if (!ok) continue;
            const uint8_t *w = want + uint64_t(j) * A.want_stride + io.lo;
            uint8_t *h = rec + uint64_t(j) * A.have_stride + io.lo;
            st_word(h, ld_word(w, io) ^ pl, io);
            st_word(h + io.hi_delta, ld_word(w + io.hi_delta, io) ^ ph, io);
        }
        return;
    }

    // a ROWS stripe with its bit on: k_heal's copy, the count of differing selected rows
    // summed here (unselected rows' flags are zero)
    if (!first && !mine) return;
    if (tid == 0) s_count = 0;
    __syncthreads();
    uint32_t c = 0;
    for (uint32_t j = tid; j < A.M; j += blockDim.x) c += marks[j] != 0;
    if (c) atomicAdd(&s_count, c);
    __syncthreads();
    const bool heal = s_count <= A.max_rows;
    if (first && tid == 0) A.action[b] = uint8_t(heal ? kHealRecovery : 0u);
    if (!heal || !ok) return;
    for (uint32_t r = r0; mine >> (r - r0); ++r) {
        if (!((mine >> (r - r0)) & 1u)) continue;
        const uint32_t j = A.rows ? rows[r] : r;
        const uint8_t *w = want + uint64_t(j) * A.want_stride + io.lo;
        uint8_t *h = rec + uint64_t(j) * A.have_stride + io.lo;
        st_word(h, ld_word(w, io), io);
        st_word(h + io.hi_delta, ld_word(w + io.hi_delta, io), io);
    }
}

// The confirm's grid (launch_locate_confirm).
bool count_grid(RobustArgs &A, dim3 &grid, uint32_t &threads) {
    threads = A.packs >= 256 ? 256u : (A.packs + 63u) / 64u * 64u;
    const uint32_t tiles = (A.packs + threads - 1) / threads;
    const uint64_t units = uint64_t(A.nsel) * tiles * A.stripes;
    A.rows_per_group = uint32_t(units / 1024 < 1 ? 1 : units / 1024 > 16 ? 16 : units / 1024);
    grid = dim3(tiles, (A.nsel + A.rows_per_group - 1) / A.rows_per_group, A.stripes);
    return grid.y <= 65535;
}

bool robust_ok(const RobustArgs &A) {
    return A.nsel >= 2 && A.nsel <= A.M && A.packs && A.N && A.t <= kRobustMaxOutliers &&
           2 * (uint64_t(A.t) + 1) <= A.nsel && A.cand && A.votes && A.outlier &&
           A.vote_bstride >= uint64_t(A.t + 1) * A.M;
}

}  // namespace

hipError_t launch_locate_find_pairs(const RobustArgs &A, hipStream_t s) {
    if (!A.stripes) return hipSuccess;
    if (!robust_ok(A)) return hipErrorInvalidValue;
    k_locate_find_pairs<<<dim3(A.stripes, A.t + 1), kFindThreads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_locate_find_pairs");
    return hipGetLastError();
}

hipError_t launch_locate_count(const RobustArgs &A0, hipStream_t s) {
    if (!A0.stripes) return hipSuccess;
    if (!robust_ok(A0) || A0.stripes > 65535) return hipErrorInvalidValue;
    RobustArgs A = A0;
    dim3 grid;
    uint32_t threads;
    if (!count_grid(A, grid, threads)) return hipErrorInvalidValue;
    k_locate_count<<<grid, threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_locate_count");
    return hipGetLastError();
}

hipError_t launch_locate_decide(const RobustArgs &A, hipStream_t s) {
    if (!A.stripes) return hipSuccess;
    if (!robust_ok(A)) return hipErrorInvalidValue;
    k_locate_decide<<<dim3(A.stripes), kFindThreads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_locate_decide");
    return hipGetLastError();
}

hipError_t launch_heal_robust(const HealRobustArgs &A0, hipStream_t s) {
    if (!A0.stripes) return hipSuccess;
    if (!robust_ok(A0) || A0.stripes > 65535 || !A0.flags || !A0.located || !A0.action || !A0.orig || !A0.rec ||
        !A0.mode || (A0.mode & ~(kHealOriginal | kHealRecovery)))
        return hipErrorInvalidValue;
    HealRobustArgs A = A0;
    dim3 grid;
    uint32_t threads;
    if (!count_grid(A, grid, threads)) return hipErrorInvalidValue;
    k_heal_robust<<<grid, threads, 0, s>>>(A);
    snprintf(launch_name_buf(), kLaunchNameBytes, "k_heal_robust");
    return hipGetLastError();
}

}  // namespace rs
