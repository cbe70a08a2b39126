// Device-side interface of the MI355X Reed-Solomon engine (host <-> kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

namespace rs {

// A contiguous range of transform rows backed by a caller buffer:
// transform row r in [row_begin, row_end) lives at base + (r - row_begin) * stride.
struct RowMap {
    const uint8_t *base = nullptr;
    uint64_t stride = 0;
    uint32_t row_begin = 0, row_end = 0;
};

// Byte layout of the caller's shard matrices (src / dst RowMaps; the work
// buffers always use whole 64-byte blocks).  Shards of any even length S:
// S / 64 whole blocks (packs 0 .. full_packs - 1 at the usual offsets), then a
// tail of t = S % 64 bytes holding tail_h = t / 2 low bytes followed by
// tail_h high bytes -- the reference's tail layout (src/engine/shards.rs:38-74,
// src/algorithm.md): tail pack p (elements 4p .. 4p + 3 of the last block) has
// its low bytes at 64 * (full_packs / 8) + 4p, its high bytes tail_h bytes
// further, and min(4, tail_h - 4p) valid elements.  io_bytes: some caller
// matrix is not 4-byte aligned (base or row stride); every caller access then
// goes byte by byte.
struct ShardFormat {
    uint32_t full_packs = 0xFFFFFFFFu;  // default: rows of whole 64-byte blocks
    uint32_t tail_h = 0;
    uint32_t io_bytes = 0;
};

// Offsets of pack pk inside a caller row: low word, high word - low word,
// valid elements, and whether the access must go byte by byte.
struct PackIO {
    uint32_t lo, hi_delta, cnt;
    bool bytes;
};
__host__ __device__ inline PackIO pack_io(const ShardFormat &f, uint32_t pk) {
    if (pk < f.full_packs) return {(pk >> 3) * 64u + (pk & 7u) * 4u, 32u, 4u, f.io_bytes != 0};
    const uint32_t p = pk - f.full_packs, e = 4u * p;
    return {(f.full_packs >> 3) * 64u + e, f.tail_h, f.tail_h > e + 4u ? 4u : f.tail_h - e, true};
}
// 2-element packs (column kernel, E = 2): pack pk holds elements 2pk, 2pk + 1 of
// a block (low bytes at 2 * (pk % 16), high bytes 32 further); tail packs as above
// with 2 elements (shards.rs:38-74).
__host__ __device__ inline PackIO pack_io2(const ShardFormat &f, uint32_t pk) {
    const uint32_t full = f.full_packs == 0xFFFFFFFFu ? 0xFFFFFFFFu : f.full_packs * 2u;
    if (pk < full) return {(pk >> 4) * 64u + (pk & 15u) * 2u, 32u, 2u, f.io_bytes != 0};
    const uint32_t e = 2u * (pk - full);
    return {(full >> 4) * 64u + e, f.tail_h, f.tail_h > e + 2u ? 2u : f.tail_h - e, true};
}
__device__ __forceinline__ uint32_t ld_half(const uint8_t *p, const PackIO &io) {
    if (!io.bytes) return *reinterpret_cast<const uint16_t *>(p);
    uint32_t v = p[0];
    if (io.cnt > 1) v |= uint32_t(p[1]) << 8;
    return v;
}
__device__ __forceinline__ void st_half(uint8_t *p, uint32_t v, const PackIO &io) {
    if (!io.bytes) {
        *reinterpret_cast<uint16_t *>(p) = uint16_t(v);
        return;
    }
    p[0] = uint8_t(v);
    if (io.cnt > 1) p[1] = uint8_t(v >> 8);
}
__device__ __forceinline__ uint32_t ld_word(const uint8_t *p, const PackIO &io) {
    if (!io.bytes) return *reinterpret_cast<const uint32_t *>(p);
    uint32_t v = 0;
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e)
        if (e < io.cnt) v |= uint32_t(p[e]) << (8 * e);
    return v;
}
__device__ __forceinline__ void st_word(uint8_t *p, uint32_t v, const PackIO &io) {
    if (!io.bytes) {
        *reinterpret_cast<uint32_t *>(p) = v;
        return;
    }
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e)
        if (e < io.cnt) p[e] = uint8_t(v >> (8 * e));
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) of kernel `fn` on the
// current device, once per device.  The attribute is per device, and one
// process may drive several GPUs through several rs_contexts (each launcher
// runs with its context's device current), so a process-wide flag would skip
// every device after the first.  `done` is the kernel's own bit set of devices
// (atomic: launchers run on many host threads).
inline hipError_t lds_attr_once(std::atomic<uint64_t> &done, const void *fn, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = dev >= 0 && dev < 64 ? uint64_t(1) << dev : 0;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && bit) done.fetch_or(bit, std::memory_order_acq_rel);
    return e;
}

// One pass of the multi-pass transform (see DESIGN.md "Pass structure").
//
// A workgroup owns one row SET x one 64-pack column SLICE.  A row set is
// 2^K transform rows whose indices differ only in bits [a, a+K):
//   row(j) = s_lo + (j << a) + (s_hi << (a + K)),  s = set index, j = local row.
// A pack is 4 GF(2^16) elements of one row: 4 low bytes at block offset 4p and
// the matching 4 high bytes at 32 + 4p (reference layout, algorithm.md:18-31).
struct PassArgs {
    uint32_t a = 0;        // stride exponent of the row set
    uint32_t nsets = 1;    // row sets of this launch (n >> K, fewer for a pruned reveal)
    uint32_t set_base = 0; // first row set of this launch (pruned decode reveal passes)
    uint32_t n = 1;        // transform size (rows per chunk)
    uint32_t packs = 0;    // packs per row (shard_bytes / 8)
    uint32_t slices = 0;   // ceil(packs / 64)
    uint32_t grid_chunks = 1;  // chunks spread over gridDim.y
    uint32_t in_chunk0 = 0;    // rows load from chunk 0 whatever the grid's chunk (LowRate: one FFT per output chunk)

    // ---- load: transform row r = row(j) + chunk * n
    RowMap src[2];
    uint32_t nsrc = 0;
    const uint32_t *rowinfo = nullptr;  // decode: bits 0-15 log factor, bit 16 = erased (row is zero)
    uint32_t load_scale = 0;            // scale loaded rows by rowinfo (erased rows load as zero)
    const uint8_t *work_in = nullptr;   // if set, rows come from work_in + r * work_stride
    uint64_t work_stride = 0;
    uint32_t in_chunks = 1;             // in-kernel XOR accumulation over chunks

    // ---- transforms
    uint32_t ifft_delta = 0, ifft_delta_step = 0;
    uint32_t fd_mode = 0;               // 0: none, 1: sum_b P_b over local bits, 2: identity + that
    const uint8_t *xor_in = nullptr;    // after fd: x ^= rows of xor_in (stride work_stride)
    uint32_t fft_delta = 0, fft_delta_step = 0;
    uint32_t out_chunks = 1;            // FFT + store repeated per output chunk

    // ---- store: transform row r = row(j) + chunk * n
    uint8_t *work_out = nullptr;        // if set, every row goes to work_out + r * work_stride
    RowMap dst;                         // else rows in [row_begin, row_end) go to dst
    uint32_t reveal = 0;                // store only erased rows, scaled by exp(65535 - factor)

    const uint32_t *tw = nullptr;       // perm tables indexed by skew index (zero table = no multiply)
    const uint32_t *lut = nullptr;      // perm tables indexed by log factor
    // tw / lut hold 8-word basis tables (rs_codec.cpp basis tables), expanded while staging
    uint32_t tab_basis = 0;
    ShardFormat fmt;                    // byte layout of src / dst (work buffers: whole blocks)

    // ---- 2-level decodes (blk_masks = 1): per block b = row >> blk_shift (b < 256),
    // zero_in bit b: the block's work_in rows are zero (never computed; load as zero);
    // keep_out bit b: the block's work_out rows are read later (others are not stored)
    // blk_uniform = 1: every row set of the launch lies inside one block (the
    // passes below the top level): one scalar test per workgroup, no store mask
    uint32_t blk_masks = 0, blk_shift = 0, blk_uniform = 0;
    uint64_t zero_in[4] = {0, 0, 0, 0};
    uint64_t keep_out[4] = {~0ull, ~0ull, ~0ull, ~0ull};

    // ---- single-pass decodes of at most kPassEvalRows work rows (fused_eval = 1):
    // every workgroup evaluates eval_poly itself (as k_eval_poly, rs_eval.hip)
    // into its LDS row info instead of reading rowinfo -- one launch, not two
    uint32_t fused_eval = 0, ev_low_rate = 0, ev_end = 0, ev_lw0 = 0;
    const uint16_t *ev_lw_fold = nullptr;      // lw_fold for 2^K points
    uint32_t ev_erased[2] = {0, 0}, ev_received[2] = {0, 0};

    // ---- the fused top pass of a multi-pass decode (bfly_prune = 1, K <= 6): its
    // local row j lies in block j (the top level's rows are the 2^K blocks of
    // 2^a rows).  zin_local bit j: block j's IFFT input is zero (zero_in);
    // need_local bit j: block j holds restored rows.  The IFFT skips the butterfly
    // groups whose 2^(b+1) rows are all zero (their outputs stay zero), the FFT
    // those that feed no needed block (their rows are never read: the FFT passes
    // below read only the needed blocks' rows)
    uint32_t bfly_prune = 0;
    uint64_t zin_local = 0, need_local = ~0ull;

    // ---- repair (reveal = 1 only): a second destination over the recovery rows'
    // work-row range, disjoint from dst; empty (row_end = 0) in every decode, whose
    // reveal stores test it with one uniform compare and never enter it
    RowMap dst2;
};
constexpr uint32_t kPassEvalRows = 64;

enum PassFlags {
    kIfft = 1,
    kFft = 2,
    // derived from PassArgs by launch_pass (compile-time kernel variants):
    kMultiIn = 4,
    kMultiOut = 8,
    kScale = 16,
    kFd = 32,
    kXorIn = 64,
    kReveal = 128,
    kEval = 256,  // fused eval_poly (PassArgs::fused_eval)
    // the IFFT's / FFT's local layer K-1 has a zero twiddle: the pass holds the
    // transform's top bit and its skew offset is 0 for every chunk of the launch
    // (rs_kernels.hip launch_k; the variants that have them)
    kZeroI = 512,
    kZeroF = 1024
};

// Launch one pass on `stream`.  K = log2(rows per set).
hipError_t launch_pass(int K, int flags, const PassArgs &args, hipStream_t stream);

// Name of the kernel the last launch_pass / launch_mono call of this thread
// launched, in rocprofv3's short form ("k_pass<8, 3, 4, 1>"): the profiler's
// records (rs_profile_collect) and the committed PMC summaries share it.
constexpr int kLaunchNameBytes = 96;
char *launch_name_buf();

// Column kernel (DESIGN.md "Column kernel"): one workgroup owns ALL n = 2^L
// transform rows of one pack (4 elements of every row), so a whole encode or
// decode runs without any cross-workgroup exchange.  Twiddles come from
// layer-ordered images: image t (transform skew offset t * n) holds, for
// layer b = 0..L-1 and group g < n / 2^(b+1), the perm table of skew index
// g * 2^(b+1) + 2^b + t * n - 1 at table slot n - n / 2^b + g.
// 2-element staged column kernels (k_mono) stage 8-word basis images and build
// their tables in LDS (rs_mono.hip Stage::kBasis) when 1; the host (rs_codec.cpp
// mono_args) hands them the matching images.  Measured no faster there, so 0;
// k_chunks always uses basis images for 2-element packs.
#ifndef RS_MONO_BASIS
#define RS_MONO_BASIS 0
#endif
// The lane kernel (rs_lane.hip) stages the 8-word basis images of its tables
// when 1 (the host, rs_codec.cpp try_lane, hands it the matching images), the
// 16-word images when 0.
// Column kernels skip the multiply of a top layer whose twiddle is zero (skew
// offset 0: rs_mono.hip run_seq zero_top) when 1.
#ifndef RS_MONO_ZERO_TOP
#define RS_MONO_ZERO_TOP 1
#endif
#ifndef RS_LANE_BASIS
#define RS_LANE_BASIS 1
#endif
enum MonoMode {
    kMonoEncodeHigh = 0,
    kMonoEncodeLow = 1,
    kMonoDecode = 2,
    // half-split transforms of 2^12 rows as two launches of 2^11-row column
    // kernels (L = 11): kMonoHalfI* run the IFFT's layers 0..10 on half
    // half0 + blockIdx.y of the rows (image ifft_img + half * ifft_img_step) and
    // store the half's rows to the work rows (dst); kMonoHalfF* load both halves'
    // work rows, run layer 11 of the IFFT (top_i), the formal derivative (Dec),
    // layer 11 of the FFT (top_f) and the FFT's layers 10..0 on half
    // out_half + blockIdx.y (image fft_img + half * fft_img_step), and store /
    // reveal its rows of dst.  *Dec: the decode's scaling (rowinfo) and reveal.
    kMonoHalfIEnc = 3,
    kMonoHalfIDec = 4,
    kMonoHalfFEnc = 5,
    kMonoHalfFDec = 6,
    // quad encode (launch_quad): a single-chunk encode of 2^L rows in 2-element
    // column packs run as the 4-element kernel of 2^(L-1) "pair rows": a pack is
    // 2 elements x rows (2q, 2q + 1), so every layer above row bit 0 multiplies 4
    // elements per table (gf_muladd4, 26 VALU) where the 2-element kernel spends
    // 2 x 24 on them; layer 0 (inside the pack) runs first / last on its own.
    kMonoQuadEnc = 7,
};
constexpr uint32_t kMonoFusedRows = 2048;  // largest work size of the fused-eval_poly decode
// The kernel arguments of every column kernel; the staged decode's kernels take
// MonoArgs (+ the erasure bitmaps), the others this core only: argument bytes
// cost launch time (≈0.4 us per KiB back to back, tools/kernarg_probe.hip).
struct MonoCore {
    uint32_t packs = 0;          // packs per row (shard_bytes / (2 * elems), rounded up)
    uint32_t packs_per_xcd = 0;  // ceil(packs / 8): workgroup b runs pack (b % 8) * packs_per_xcd + b / 8
    RowMap src[2];               // transform rows to load (others are zero)
    uint32_t nsrc = 0;
    RowMap dst;                  // transform rows to store (decode: erased originals only)
    uint32_t chunks = 1;         // high: IFFT chunks XOR-folded; low: FFT output chunks
    const uint32_t *img = nullptr;  // twiddle images of this L, image t at img + t * img_words
    uint64_t img_words = 0;         // (n - 1) * table words (20, or 16 in the 2-element format)
    uint32_t elems = 4;             // pack format: 4 or 2 elements per pack (rs_mono.hip Fmt)
    uint32_t ifft_img = 0, ifft_img_step = 0;  // image of IFFT chunk c: ifft_img + c * ifft_img_step
    uint32_t fft_img = 0, fft_img_step = 0;
    const uint32_t *rowinfo = nullptr;  // decode: bits 0-15 log factor, bit 16 erased
    const uint32_t *lut = nullptr;      // perm tables by log factor (Engine::mul semantics; format of elems)
    // decode with eval_poly fused into the staged kernel (every workgroup
    // evaluates it; no rowinfo; MonoArgs::erased / received)
    uint32_t fused_eval = 0, low_rate = 0, end = 0, lw0 = 0;
    // split plan (mono_split(L)): every restored row lies in half out_half of the 2^L work rows
    uint32_t split = 0, out_half = 0;
    ShardFormat fmt;  // byte layout of src / dst
    const uint16_t *lw_fold = nullptr;
    // a batch of stripes of one shape in one launch (staged kernel, grid.y =
    // stripes): stripe b's rows sit b * *_bstride bytes after the base
    // pointers (read only by the batch instantiation)
    uint32_t stripes = 1;
    uint64_t src_bstride[2] = {0, 0}, dst_bstride = 0;
    // half-split kernels (kMonoHalf*): first half of the launch, halves whose work
    // rows are all zero (bit h; not read), layer-11 perm tables of the IFFT / FFT
    uint32_t half0 = 0, zero_halves = 0;
    const uint32_t *top_i = nullptr, *top_f = nullptr;
};
// The staged single-chunk encodes take the fields their prologue needs as plain
// leading kernel parameters, 14 dwords in this order (no padding), followed by the
// MonoCore: gfx950 preloads argument dwords into the user SGPRs at wave launch, plain
// parameters only, and 14 are free beside the argument pointer (rs_mono.hip k_mono's
// encode entry).  The first two lines let the row loads go (one source map: nsrc = 1),
// the third the table loads.
struct MonoLead {
    const uint8_t *src;
    uint64_t src_stride;
    uint32_t src_begin, src_end, packs, packs_per_xcd, full_packs;
    uint32_t tail_io;  // ShardFormat: tail_h | io_bytes << 16
    const uint32_t *img;
    uint32_t img_words;
    uint32_t imgs;  // ifft_img | fft_img << 16
};
static_assert(sizeof(MonoLead) == 56, "14 dwords, no padding");
// The dense form of that entry (rs_mono.hip k_mono_dense; rs_mono_dense.hpp
// mono_dense_ok decides on the host): every transform row [0, 2^L) is a row of the
// one source map and of the destination map, in full, 4-byte aligned packs.  The row
// ranges and the shard format say nothing then, and their four dwords carry the
// destination map instead: a single-stripe launch reads no argument from memory.
struct MonoLeadDense {
    const uint8_t *src;
    uint64_t src_stride;  // (both strides < 2^24, 2^L rows of them <= 2^32 bytes: mono_dense_ok)
    uint8_t *dst;
    uint64_t dst_stride;
    uint32_t packs, packs_per_xcd;
    const uint32_t *img;
    uint32_t img_words;
    uint32_t imgs;  // ifft_img | fft_img << 16
};
static_assert(sizeof(MonoLeadDense) == 56, "14 dwords, no padding");
// launch_mono's mode + kMonoNoDense: the general entry also where the dense one could run
// (rs_mono_enable + 8192, RS_MI355X_DENSE=0)
constexpr int kMonoNoDense = 0x100;
// launches of the dense entry by this process so far (tests, A/B: the profile records
// name both forms k_mono<...>, as the traces of the general entry always have)
uint64_t mono_dense_launches();
struct MonoArgs : MonoCore {
    // fused-eval_poly decode: erased / received bits of the 2^L work rows, as in EvalArgs
    uint32_t erased[kMonoFusedRows / 32] = {}, received[kMonoFusedRows / 32] = {};
};
// hipErrorNotSupported: no column kernel for this L (7 <= L <= 12 are built).
// split_img (encodes): the context's split images (rs_stage_map.hpp SplitImage, image t
// at split_img + t * SplitImage<10>::kWords); where the dense entry would run a launch
// of 2^10 rows in 2-element packs, one stripe, its split form runs instead (rs_mono.hip
// k_mono_split).  nullptr: never.
hipError_t launch_mono(int mode, int L, const MonoArgs &A, hipStream_t stream, const uint32_t *split_img = nullptr);
// launches of the split form so far (each also counts in mono_dense_launches)
uint64_t mono_split_launches();
// Repair (rs_repair_device*): the decode kernels with a second destination map,
// dst2 over the recovery rows' work-row range (dst: the originals').  A row is
// stored to the map that holds it when it is erased; rows of neither map (the
// HighRate padding [M, chunk)) stay unwritten.  Either map may be empty
// (row_begin = row_end = 0).  These are instantiations of their own
// (k_mono_repair, built in rs_repair.hip from rs_mono.hip's body): the decode's
// kernels and their arguments stay as they are.
struct MonoArgs2 : MonoArgs {
    RowMap dst2;
    uint64_t dst2_bstride = 0;
};
// kMonoDecode: the staged fused-eval_poly kernel (7 <= L <= 11; plain or split
// plan, stripes >= 1 as grid.y) or the unstaged one (L = 12, rowinfo).
hipError_t launch_mono_repair(int L, const MonoArgs2 &A, hipStream_t stream);
// kMonoHalfFDec with two destinations (launch_mono_half's second launch).
hipError_t launch_mono_half_repair(uint32_t halves, const MonoArgs2 &A, hipStream_t stream);
// The staged batch decode with one erasure pattern PER STRIPE (k_mono_masks): the
// patterns come from a device array of descriptors instead of the kernel arguments.
// Descriptor of stripe b, at desc + b * desc_words (32-byte aligned, so a wave's
// words are one aligned scalar load): word 0 = skip (the stripe's workgroups
// return at once: nothing missing, or undecodable), words 1..7 unused, then for
// each wave w of the workgroup (128 work rows each) 8 words: the erased bits of
// work rows 128 w .. 128 w + 127, then their received bits (as MonoArgs::erased /
// received).
constexpr uint32_t kMaskDescHead = 8;
constexpr uint32_t mask_desc_words(uint32_t L) { return kMaskDescHead + 8u * ((1u << L) / 128u); }
struct MonoMaskArgs : MonoCore {
    const uint32_t *desc = nullptr;
    uint32_t desc_words = 0;
};
// Plain plan, fused eval_poly, grid.y = A.stripes (>= 1); 7 <= L <= 11, elems 2 or 4.
hipError_t launch_mono_masks(int L, const MonoMaskArgs &A, hipStream_t stream);
// The repair of such a batch (k_mono_repair_masks, built in rs_repair.hip): the
// same descriptors (a stripe's erased bits cover the recovery rows' work rows too)
// and the second destination map of MonoArgs2, both maps whole.
struct MonoMaskArgs2 : MonoMaskArgs {
    RowMap dst2;
    uint64_t dst2_bstride = 0;
};
hipError_t launch_mono_repair_masks(int L, const MonoMaskArgs2 &A, hipStream_t stream);
// Multi-chunk encodes of 2^L rows, 2 <= L <= 7 (rs_chunks.hip): HighRate (high:
// A.chunks input chunks, images ifft_img + c * ifft_img_step, fft_img) or
// LowRate (A.chunks output chunks, images ifft_img, fft_img + c * fft_img_step);
// src[0] / dst, one stripe, A.chunks >= 2, elems 2 or 4.
bool chunks_supported(int L);
// pw: packs per wave (1, 2, 4): each wave transforms its chunks for pw packs
// with one staging of the chunk's tables (A.packs_per_xcd is recomputed).
hipError_t launch_chunks(int L, bool high, const MonoCore &A, hipStream_t stream, int pw = 1);
// kMonoHalf* modes: L = 11 only, one stripe, grid.y = halves (launch_mono_half).
hipError_t launch_mono_half(int mode, uint32_t halves, const MonoArgs &A, hipStream_t stream);
// Quad encode of 2^L rows (kMonoQuadEnc; quad_supported(L)): packs / fmt / rows of
// the 2-element format; img = the 4-element images of 2^L rows offset by 2^(L-1)
// tables (layer 0 skipped), img_words = (2^L - 1) * 20; lut = the 2-element images
// of 2^L rows (their layer-0 tables); one chunk; stripes for a batch.
bool quad_supported(int L);
hipError_t launch_quad(int L, const MonoArgs &A, hipStream_t stream);
// Variant launch_mono picks: LDS-staged twiddles (single chunk, 2 rows per
// lane, L <= 11); fused_eval and stripes > 1 require it.
bool mono_staged(int L, uint32_t chunks);
// Decodes of 2^L work rows (L in 9..11) whose restored rows all lie in one half
// may use the split plan (MonoArgs::split): the FFT below the top layer runs
// only on that half.
bool mono_split(int L);
int mono_rows_log2_per_lane(int L, uint32_t chunks);

// Lane column kernel (rs_lane.hip): the single-chunk encode of 2^L rows
// (lane_supported(L): 8 <= L <= 10) in 2-element packs with one row per thread;
// takes the column kernel's arguments (elems = 2, chunks = 1; stripes for a batch).
bool lane_supported(int L);
hipError_t launch_lane(int L, const MonoCore &A, hipStream_t stream);

// eval_poly for a decode (src/engine/utils.rs:20-31) reduced to 2^u points
// (DESIGN.md "eval_poly"): erasure vector -> per-row log factors.
//   row r < 2^u: erased bit e(r) (erasure-vector entry) and received bit.
//   low_rate: the erasure vector is also 1 on [2^u, 65536) (rate_low.rs:196).
//   end: recovery_end / original_end.
// Output rowinfo[r] = log factor | (received ? 0 : 0x10000).
// Rows' bits travel in the kernel arguments when 2^u <= kEvalInlineRows (no
// copy, no extra launch), else in a device byte array (bit0 erased, bit1 received).
constexpr uint32_t kEvalInlineRows = 8192;
struct EvalArgs {
    uint32_t u = 0, low_rate = 0, end = 0, lw0 = 0;
    const uint16_t *lw_fold = nullptr;  // lw_fold for this u (2^u entries)
    uint32_t *rowinfo = nullptr;
    const uint8_t *state = nullptr;     // 2^u > kEvalInlineRows only
    uint32_t erased[kEvalInlineRows / 32] = {};
    uint32_t received[kEvalInlineRows / 32] = {};
};
hipError_t launch_eval_poly(const EvalArgs &A, hipStream_t stream);

// ---- update (rs_update_device*, rs_update.hip; DESIGN.md "Update") ----------
// Coefficient step.  launch_update_unit writes the unit stripe into zeroed
// rows of `stride` = 64 * ceil(count / 32) bytes: element c of row index[c] = 1
// (low byte 1 at offset c % 32 of block c / 32).  launch_update_log turns the
// encode of that stripe (`coef`, rows of `stride` bytes) into logs[j * count + c]
// = log of element c of recovery row j; element 0 becomes kUpdateNoCoef.
constexpr uint32_t kUpdateNoCoef = 65535;  // (log[0] of the host table: no multiplier has this log)
hipError_t launch_update_unit(uint8_t *unit, uint64_t stride, const uint32_t *index, uint32_t count, hipStream_t stream);
hipError_t launch_update_log(const uint8_t *coef, uint64_t stride, uint32_t rows, uint32_t count,
                             const uint16_t *log_table, uint16_t *logs, hipStream_t stream);
// The direct update (k_update): for every selected recovery row j (rows[r], r <
// nsel; rows = nullptr: row r) and every pack, recovery_j ^= XOR_c delta_c *
// exp(logs[j * count + c]), delta_c = old_c ^ new_c (old = nullptr: new_c).
// grid = (pack tiles, row groups, stripes); the deltas are formed once per
// workgroup and, for count <= kUpdateTile, stay in registers across its rows.
constexpr uint32_t kUpdateTile = 16;
struct UpdateArgs {
    const uint8_t *old_rows = nullptr, *new_rows = nullptr;  // count rows each
    uint8_t *rec = nullptr;
    uint64_t old_stride = 0, new_stride = 0, rec_stride = 0;
    uint64_t old_bstride = 0, new_bstride = 0, rec_bstride = 0;  // stripe b: + b * bstride
    uint32_t packs = 0, count = 0, nsel = 0, stripes = 1;
    uint32_t rows_per_group = 1;
    const uint32_t *rows = nullptr;
    const uint16_t *logs = nullptr;  // 4-byte aligned
    const uint32_t *lut = nullptr;   // perm tables by log factor (rs_context::d_lut)
    ShardFormat fmt;
};
hipError_t launch_update(const UpdateArgs &A, hipStream_t stream);
// The same with a list per stripe (k_update_lists, rs_update_device_batch_lists): stripe b
// overwrites originals index[b * index_pitch + c], c < counts[b] (0: the stripe is left alone,
// nothing of it read or written), and touches recovery row j only where sel[b * M + j] != 0
// (sel = nullptr: every row).  logs is the table over every original, logs[j * N + i] =
// log G[j][i] (launch_locate_log), zero coefficients as kUpdateNoCoef.  grid = (pack tiles,
// groups of rows of M, stripes); stripes <= 65535.
struct UpdateListsArgs {
    const uint8_t *old_rows = nullptr, *new_rows = nullptr;  // a row per index, stripe b at b * bstride
    uint8_t *rec = nullptr;
    uint64_t old_stride = 0, new_stride = 0, rec_stride = 0;
    uint64_t old_bstride = 0, new_bstride = 0, rec_bstride = 0;  // stripe b: + b * bstride
    uint32_t packs = 0, index_pitch = 0, N = 0, M = 0, stripes = 1;
    uint32_t rows_per_group = 1;
    const uint32_t *counts = nullptr;  // stripes words
    const uint32_t *index = nullptr;   // stripes x index_pitch words (index_pitch >= every count)
    const uint8_t *sel = nullptr;      // stripes x M bytes, 4-byte aligned
    const uint16_t *logs = nullptr;    // 4-byte aligned
    const uint32_t *lut = nullptr;     // perm tables by log factor (rs_context::d_lut)
    ShardFormat fmt;
};
hipError_t launch_update_lists(const UpdateListsArgs &A, hipStream_t stream);
// Row-wise XOR over a row list (the re-encode route's two ends): for r < nrows,
// out row (out_list ? list[r] : r) = a row (a_list ? list[r] : r) ^ b row (b_list
// ? list[r] : r); b = nullptr: a copy of the a row.  list = nullptr: row r everywhere.
struct UpdateXorArgs {
    uint8_t *out = nullptr;
    const uint8_t *a = nullptr, *b = nullptr;
    uint64_t out_stride = 0, a_stride = 0, b_stride = 0;
    const uint32_t *list = nullptr;
    uint32_t out_list = 0, a_list = 0, b_list = 0;
    uint32_t nrows = 0, packs = 0;
    ShardFormat fmt;
};
hipError_t launch_update_xor(const UpdateXorArgs &A, hipStream_t stream);

// ---- verify (rs_verify_device*, rs_verify.hip; DESIGN.md "Verify") ----------
// The fused route (k_mono_verify): the staged single-chunk column encode whose
// store_col compares instead of storing.  dst is the caller's recovery matrix,
// narrowed to the span of the selected rows; a lane loads the caller's word from
// the address it would have stored to and, where it differs from the encoded
// word, stores the byte 1 to flags[stripe * flag_bstride + (r - dst.row_begin)].
// sel (nullptr: every row of dst): sel[r - dst.row_begin] != 0 = row r is
// compared; the others are never read.  Row dst.row_begin must be selected (lanes
// without a row of their own read it and discard it).  The kernel takes the
// encode's MonoCore, not MonoArgs: the encodes have no erasure bitmaps, and
// argument bytes cost launch time.
struct MonoVerifyArgs : MonoCore {
    uint8_t *flags = nullptr;
    uint64_t flag_bstride = 0;
    const uint8_t *sel = nullptr;
};
// Staged kernel only (mono_staged(L, 1): 7 <= L <= 11), A.chunks = 1, elems 2 or
// 4, grid.y = A.stripes (>= 1).  The staged body is the same for both rates (they
// differ in the images the host names), so one kernel per (L, elems) serves both.
hipError_t launch_mono_verify(int L, const MonoVerifyArgs &A, hipStream_t stream);
// The fused route with one selection PER STRIPE (k_mono_verify_masks, rs_verify_device_batch_masks):
// dst is narrowed to the union of the stripes' selected spans, sel (not nullptr) points at
// stripe 0's selection byte of row dst.row_begin and stripe b's bytes sit b * sel_bstride
// further.  Row dst.row_begin need not be selected in every stripe, so the row a lane
// without a row of its own reads and discards is the stripe's: first[b] = the stripe's
// first selected row minus dst.row_begin, or kVerifyNoRow where the stripe selects
// nothing -- its workgroups return before their first row load.
constexpr uint32_t kVerifyNoRow = 0xFFFFFFFFu;
struct MonoVerifyMaskArgs : MonoVerifyArgs {
    uint64_t sel_bstride = 0;
    const uint32_t *first = nullptr;  // one word per stripe
    // some first[b] is kVerifyNoRow: only then do the workgroups wait for their word
    // ahead of the row loads (a dependent scalar load in front of every workgroup's
    // prologue otherwise); without one the word is first needed behind them
    uint32_t has_empty = 0;
};
// As launch_mono_verify; one launch for the A.stripes <= 65535 stripes.
hipError_t launch_mono_verify_masks(int L, const MonoVerifyMaskArgs &A, hipStream_t stream);
// The unfused route's compare (k_verify_rows): for r < nrows and every pack, row
// j = rows ? rows[r] : r of `want` (the encode in scratch) against row j of `have`
// (the caller's recovery matrix), both in the layout of fmt; a difference stores
// the byte 1 to flags[stripe * flag_bstride + j].  grid = (pack tiles, nrows, stripes).
struct VerifyRowsArgs {
    const uint8_t *want = nullptr, *have = nullptr;
    uint64_t want_stride = 0, have_stride = 0;
    uint64_t want_bstride = 0, have_bstride = 0;  // stripe b: + b * bstride
    const uint32_t *rows = nullptr;
    uint32_t nrows = 0, packs = 0, stripes = 1;
    uint8_t *flags = nullptr;
    uint64_t flag_bstride = 0;
    ShardFormat fmt;
};
hipError_t launch_verify_rows(const VerifyRowsArgs &A, hipStream_t stream);
// The compare with one row list PER STRIPE (k_verify_rows_masks): stripe b's rows are
// rows[b * list_stride + r], r < counts[b]; nrows = the largest count (the grid's y:
// workgroups past a stripe's count leave at once, a stripe with count 0 reads nothing).
struct VerifyRowsMaskArgs : VerifyRowsArgs {
    uint64_t list_stride = 0;
    const uint32_t *counts = nullptr;  // one word per stripe
};
hipError_t launch_verify_rows_masks(const VerifyRowsMaskArgs &A, hipStream_t stream);

// ---- locate (rs_locate_device*, rs_locate.hip; DESIGN.md "Locate") ----------
// The coefficient step over a slab of consecutive originals i0 .. i0 + count - 1:
// launch_locate_unit writes the slab's unit stripe into zeroed rows of `stride` =
// 64 * ceil(count / 32) bytes (element c of row i0 + c = 1); launch_locate_log
// turns its encode into logs[j * pitch + i0 + c] (pitch = original_count: the
// slabs fill one M x N table), element 0 as kUpdateNoCoef.
hipError_t launch_locate_unit(uint8_t *unit, uint64_t stride, uint32_t i0, uint32_t count, hipStream_t stream);
hipError_t launch_locate_log(const uint8_t *coef, uint64_t stride, uint32_t rows, uint32_t i0, uint32_t count,
                             uint32_t pitch, const uint16_t *log_table, uint16_t *logs, hipStream_t stream);
// The values of located[] below zero (include/rs_mi355x.h RS_LOCATE_*).
constexpr int32_t kLocateClean = -1, kLocateRows = -2, kLocateUnknown = -3;
// After the unfused verify of `stripes` stripes (want: the encode in scratch, have:
// the caller's recovery matrix, flags: what k_verify_rows stored over zeroes).
// launch_locate_find (grid = stripes) writes every located[b]: kLocateClean /
// kLocateRows from the flags, else the candidate original or kLocateUnknown.
// launch_locate_confirm (grid = pack tiles, row groups, stripes <= 65535) checks
// the candidates over every selected row and pack and stores kLocateUnknown where
// one is refuted.  rows: the nsel >= 2 selected rows in order (nullptr: every row).
struct LocateArgs {
    const uint8_t *want = nullptr, *have = nullptr;
    uint64_t want_stride = 0, have_stride = 0;
    uint64_t want_bstride = 0, have_bstride = 0;  // stripe b: + b * bstride
    const uint32_t *rows = nullptr;
    uint32_t nsel = 0, packs = 0, stripes = 1;
    uint32_t N = 0, M = 0;  // original_count, recovery_count
    uint32_t rows_per_group = 1;
    const uint8_t *flags = nullptr;
    uint64_t flag_bstride = 0;
    int32_t *located = nullptr;
    const uint16_t *logs = nullptr;       // log G[j][i] at j * N + i, 4-byte aligned
    const uint16_t *log_table = nullptr;  // log of every element (rs_context::d_log)
    const uint32_t *lut = nullptr;        // perm tables by log factor (rs_context::d_lut)
    ShardFormat fmt;
    uint32_t *differ = nullptr;  // a heal's: the find stores stripe b's count of differing selected rows
};
hipError_t launch_locate_find(const LocateArgs &A, hipStream_t stream);
hipError_t launch_locate_confirm(const LocateArgs &A, hipStream_t stream);
// The two launches with one row list PER STRIPE (k_locate_find_masks,
// k_locate_confirm_masks; rs_locate_device_batch_masks): stripe b's selected rows are
// rows[b * list_stride + r], r < counts[b], in order; nsel = the largest count (the
// confirm's grid).  A stripe with counts[b] < 2 is skipped: the find stores
// kLocateSkipped, the confirm leaves, neither reads a row of it.
constexpr int32_t kLocateSkipped = -4;  // include/rs_mi355x.h RS_LOCATE_SKIPPED
struct LocateMaskArgs : LocateArgs {
    uint64_t list_stride = 0;
    const uint32_t *counts = nullptr;  // one word per stripe
};
hipError_t launch_locate_find_masks(const LocateMaskArgs &A, hipStream_t stream);
hipError_t launch_locate_confirm_masks(const LocateMaskArgs &A, hipStream_t stream);

// ---- degraded locate (rs_locate_device_degraded*, rs_locate.hip; DESIGN.md "Degraded locate") ----
// map: N words, map[p] = p where original p is present, else N + the reference
// recovery row that stands in for it (an information position either way).
// launch_locate_unit_degraded is launch_locate_unit over information positions i0 ..
// i0 + count - 1: element c of the shard map[i0 + c] names = 1, in zeroed unit
// matrices of `stride` >= 64 * ceil(count / 32) bytes per row.  launch_locate_rename
// (one thread per stripe, after the confirm) replaces located[b] = p in [0, N) by map[p].
hipError_t launch_locate_unit_degraded(uint8_t *unit_orig, uint8_t *unit_rec, uint64_t stride, const int32_t *map,
                                       uint32_t N, uint32_t i0, uint32_t count, hipStream_t stream);
hipError_t launch_locate_rename(int32_t *located, const int32_t *map, uint32_t N, uint32_t stripes,
                                hipStream_t stream);

// ---- heal (rs_heal_device*, rs_locate.hip; DESIGN.md "Heal") -----------------
// After the find (with `differ`) and the confirm of the same LocateArgs, while the
// encode is still in `want`.  launch_heal (the confirm's grid) writes every
// action[b] and, where action[b] != 0, the stripe: kHealOriginal (located[b] = i >= 0
// and the mode bit): original i ^= D_j0 / G[j0][i] over every pack; kHealRecovery
// (located[b] = kLocateRows, the mode bit, differ[b] <= max_rows): every flagged
// selected row of `rec` = that row of `want`.  rec is the matrix `have` names.
constexpr uint32_t kHealOriginal = 1, kHealRecovery = 2;
struct HealArgs : LocateArgs {
    uint8_t *orig = nullptr, *rec = nullptr;
    uint64_t orig_stride = 0, orig_bstride = 0;
    uint32_t mode = 0, max_rows = 0;
    uint8_t *action = nullptr;  // one byte per stripe
};
hipError_t launch_heal(const HealArgs &A, hipStream_t stream);
// launch_heal with one row list PER STRIPE (k_heal_masks; rs_heal_device_batch_masks,
// DESIGN.md §4.4l), after launch_locate_find_masks (with `differ`) and
// launch_locate_confirm_masks of the same arguments, on the latter's grid: the row
// whose D gives e is the stripe's own rows[b * list_stride], and a kLocateRows stripe
// walks its own counts[b] entries.  A skipped stripe gets action[b] = 0 and nothing of
// it is read.  Derived from LocateMaskArgs, so that the three *_masks launches of a
// group take one object; the heal's fields are HealArgs'.
struct HealMaskArgs : LocateMaskArgs {
    uint8_t *orig = nullptr, *rec = nullptr;
    uint64_t orig_stride = 0, orig_bstride = 0;
    uint32_t mode = 0, max_rows = 0;
    uint8_t *action = nullptr;  // one byte per stripe
};
hipError_t launch_heal_masks(const HealMaskArgs &A, hipStream_t stream);

// ---- degraded heal (rs_heal_device_degraded*, rs_locate.hip; DESIGN.md "Degraded heal") ----
// launch_locate_log_rows is launch_locate_log over a row list: logs[r * pitch + i0 + c]
// = log of element c of row rows[r] of `coef`, r < nrows -- the table log U[r][q], m x N,
// from the restored rows (rows: the missing originals) of the unit stripe's repair.
// launch_heal_degraded runs between the confirm and the rename of a degraded locate's
// group, after a find with `differ`: located[b] is still an information position q and
// `want` the completed stripe's encode.  It writes every action[b] and, where action[b]
// != 0, the stripe: a located q whose shard map[q] is an original (kHealOriginal and the
// mode bit) or a reference row (kHealRecovery and the mode bit): that shard ^= e = D_j0 /
// T[j0][q], and row miss[r] of `restored` ^= U[r][q] * e for r < m; kLocateRows (the mode
// bit, differ[b] <= max_rows): launch_heal's copy over the check rows.  grid = (the
// confirm's pack tiles, row groups over max(m, nsel), stripes); a located stripe's m
// restored rows are dealt round the row groups.
struct HealDegradedArgs : HealArgs {
    const int32_t *map = nullptr;    // N words (launch_locate_unit_degraded)
    const uint32_t *miss = nullptr;  // the m missing originals in order
    const uint16_t *logu = nullptr;  // log U[r][q] at r * N + q, 4-byte aligned
    uint32_t m = 0;
    uint8_t *restored = nullptr;
    uint64_t restored_stride = 0, restored_bstride = 0;
};
hipError_t launch_locate_log_rows(const uint8_t *coef, uint64_t stride, const uint32_t *rows, uint32_t nrows,
                                  uint32_t i0, uint32_t count, uint32_t pitch, const uint16_t *log_table,
                                  uint16_t *logs, hipStream_t stream);
hipError_t launch_heal_degraded(const HealDegradedArgs &A, hipStream_t stream);

// ---- robust locate (rs_locate_device_robust*, rs_locate_robust.hip; DESIGN.md "Robust locate") ----
// After the unfused verify, as the locate's launches, with t <= kRobustMaxOutliers
// and 2 (t + 1) <= nsel.  launch_locate_find_pairs (grid = stripes x pairs) writes every
// located[b] -- kLocateClean / kLocateRows from the flags, else kLocateUnknown -- and
// cand[b * (kRobustMaxOutliers + 1) + p] for p <= t: the original that pair p of the
// selected-row list names, or -1.  launch_locate_count (the confirm's grid) stores
// the byte 1 to votes[b * vote_bstride + p * M + j] where selected row j disagrees
// with candidate p (e from the candidate's own reference row, sel[2p]); votes are
// zeroed ahead of it.  launch_locate_decide (grid = stripes) stores the first
// candidate with at most t bytes set to located[b] and those bytes to the zeroed
// outlier[b * outlier_bstride + j].
constexpr uint32_t kRobustMaxOutliers = 7;  // include/rs_mi355x.h RS_LOCATE_MAX_OUTLIERS
struct RobustArgs : LocateArgs {
    uint32_t t = 0;  // max_outliers
    int32_t *cand = nullptr;
    uint8_t *votes = nullptr;
    uint64_t vote_bstride = 0;  // >= (t + 1) * M
    uint8_t *outlier = nullptr;
    uint64_t outlier_bstride = 0;
};
hipError_t launch_locate_find_pairs(const RobustArgs &A, hipStream_t stream);
hipError_t launch_locate_count(const RobustArgs &A, hipStream_t stream);
hipError_t launch_locate_decide(const RobustArgs &A, hipStream_t stream);

// ---- robust heal (rs_heal_device_robust*, rs_locate_robust.hip; DESIGN.md "Robust heal") ----
// After launch_locate_decide of the same RobustArgs, while the encode is still in
// `want`.  launch_heal_robust (the confirm's grid) writes every action[b], a bit set,
// and the stripe: located[b] = i >= 0: with e = D_r / G[r][i] (r: the first selected
// row with outlier[b][r] = 0), kHealOriginal (the mode bit): original i ^= e over every
// pack; kHealRecovery (the mode bit, some outlier byte set): every row j of `rec` with
// outlier[b][j] set = row j of `want` ^ G[j][i] * e.  located[b] = kLocateRows: as
// launch_heal, the count of differing rows summed from the flags.  rec is the matrix
// `have` names.
struct HealRobustArgs : RobustArgs {
    uint8_t *orig = nullptr, *rec = nullptr;
    uint64_t orig_stride = 0, orig_bstride = 0;
    uint32_t mode = 0, max_rows = 0;
    uint8_t *action = nullptr;  // one byte per stripe
};
hipError_t launch_heal_robust(const HealRobustArgs &A, hipStream_t stream);

// x[rows] *= exp(log_m) over `blocks` 64-byte blocks.
hipError_t launch_mul(uint8_t *rows, uint64_t blocks, const uint32_t *lut_entry, hipStream_t stream);

// out[q] = in[q] ^ XOR_{b: q_b = 0, 2^b < rows} in[q | 2^b]  (formal derivative, closed form)
hipError_t launch_formal_derivative(const uint8_t *in, uint8_t *out, uint32_t rows, uint64_t row_bytes,
                                    hipStream_t stream);

}  // namespace rs
