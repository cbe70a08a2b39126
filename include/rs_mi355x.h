/*
 * rs_mi355x.h -- C ABI of the MI355X (gfx950) Reed-Solomon GF(2^16) engine.
 *
 * Drop-in boundary for AndersTrier/reed-solomon-simd v3.1.0 (reference mounted
 * at /root/reference; paths below are relative to it).  Plain pointers and
 * sizes only; device pointers are HIP device allocations, `stream` is a
 * hipStream_t passed as void* (NULL = default stream).
 *
 *   reference item                                   replaced by
 *   -----------------------------------------------  ------------------------------
 *   Error enum + fields        src/lib.rs:48-142     rs_status / rs_error
 *   encode()/decode()          src/lib.rs:251-353    rs_encode / rs_decode (host buffers)
 *   ReedSolomonEncoder         src/reed_solomon.rs:13-81
 *     ::new / ::reset / ::supports                    rs_encoder_new / _reset / rs_supports
 *     ::add_original_shard                            rs_encoder_add_original_shard
 *     ::encode -> EncoderResult                       rs_encoder_encode
 *     EncoderResult::recovery  src/encoder_result.rs:17-33   rs_encoder_recovery
 *     EncoderResult Drop (reset_received)             rs_encoder_result_drop
 *   ReedSolomonDecoder         src/reed_solomon.rs:83-183
 *     ::add_original_shard / ::add_recovery_shard     rs_decoder_add_*_shard
 *     ::decode -> DecoderResult                       rs_decoder_decode
 *     DecoderResult::restored_original src/decoder_result.rs:17-33  rs_decoder_restored_original
 *   DefaultRate / HighRate / LowRate  src/rate/rate_*.rs  rs_rate (RS_RATE_DEFAULT/HIGH/LOW)
 *   trait Engine               src/engine.rs:234-291
 *     fft / ifft (ShardsRefMut, pos, size, trunc, skew_delta)  rs_engine_fft / rs_engine_ifft
 *     mul(x, log_m)                                   rs_engine_mul
 *     eval_poly(erasures, truncated)                  rs_engine_eval_poly (host array)
 *   tables::get_exp_log / get_skew  src/engine/tables.rs:98-165  rs_table_exp/log/skew
 *
 * Device-resident batch entry points (the performance path; no reference
 * counterpart because the reference engine only sees host slices):
 *   rs_encode_device / rs_decode_device (+ _strided, + _batch: many
 *   stripes of one shape in one launch; rs_decode_device_batch_masks: the
 *   batch decode with an erasure pattern per stripe)
 *   rs_repair_device (+ _strided, + _batch; rs_repair_device_batch_masks: a
 *   pattern per stripe): the decode that also rebuilds missing recovery shards
 *   rs_update_device (+ _batch; rs_update_device_batch_lists: an index list per
 *   stripe): a partial-stripe write applied to the recovery shards in place,
 *   from the changed originals' deltas alone
 *   rs_verify_device (+ _batch): which recovery shards no longer agree with the
 *   originals
 *   rs_locate_device (+ _batch): the verify that also names the one corrupt
 *   original of a stripe whose recovery shards all disagree
 *   rs_locate_device_robust (+ _batch): the locate that tolerates, and names, a
 *   few corrupt recovery shards beside the corrupt original
 *   rs_heal_device (+ _batch; rs_heal_device_batch_masks: a recovery-row mask
 *   per stripe): the locate that also writes the correction, to the
 *   located original or to the differing recovery rows, with no host round trip
 *
 * Thread-safety: a context may be shared by threads (like DefaultEngine:
 * Send + Sync, src/lib.rs:385-409): calls on one context are serialized on the
 * host by an internal mutex, and the device scratch is kept per (context,
 * stream), so calls enqueued on different streams may execute concurrently on
 * the device.  Do not destroy a stream while calls on it are in flight and
 * then pass a new stream that reuses its handle.  A context keeps the scratch
 * of at most RS_MAX_STREAM_WORKSPACES streams (device buffers sized to the
 * largest call made on each, plus pinned staging); a call on a further stream
 * takes over the least recently used stream's scratch (buffers kept, no free)
 * after waiting for that stream's last call -- by an event recorded at the end
 * of each call once 8 or more streams are in use, else by synchronizing the
 * device.  rs_release_stream_scratch frees one stream's scratch at once (call
 * it before destroying a stream the context has seen).  Single-level HighRate
 * encodes with several chunks and few packs spread the chunks over the grid,
 * with a work buffer of about the input's size, only up to 256 MiB of it; larger
 * ones run the chunks in sequence without one.  Every entry point runs on
 * the context's device and restores the calling thread's current device.  An
 * encoder/decoder handle is used by one thread at a time (like
 * &mut ReedSolomonEncoder).
 */
#ifndef RS_MI355X_H
#define RS_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error codes, one per reference Error variant (src/lib.rs:48-142). */
typedef enum rs_status {
    RS_OK = 0,
    RS_ERR_DIFFERENT_SHARD_SIZE = 1,            /* shard_bytes, got */
    RS_ERR_DUPLICATE_ORIGINAL_SHARD_INDEX = 2,  /* index */
    RS_ERR_DUPLICATE_RECOVERY_SHARD_INDEX = 3,  /* index */
    RS_ERR_INVALID_ORIGINAL_SHARD_INDEX = 4,    /* original_count, index */
    RS_ERR_INVALID_RECOVERY_SHARD_INDEX = 5,    /* recovery_count, index */
    RS_ERR_INVALID_SHARD_SIZE = 6,              /* shard_bytes */
    RS_ERR_NOT_ENOUGH_SHARDS = 7,               /* original_count, original_received_count, recovery_received_count */
    RS_ERR_TOO_FEW_ORIGINAL_SHARDS = 8,         /* original_count, original_received_count */
    RS_ERR_TOO_MANY_ORIGINAL_SHARDS = 9,        /* original_count */
    RS_ERR_UNSUPPORTED_SHARD_COUNT = 10,        /* original_count, recovery_count */
    /* not in the reference: */
    RS_ERR_DEVICE = 100,                        /* HIP runtime failure (message via rs_last_device_error) */
    RS_ERR_INVALID_ARGUMENT = 101               /* null handle / pointer, or unsupported device-API layout */
} rs_status;

/* Error payload; fields not used by a variant are 0.  Field names follow the
 * reference variants' fields. */
typedef struct rs_error {
    int32_t code; /* rs_status */
    uint64_t original_count;
    uint64_t recovery_count;
    uint64_t shard_bytes;
    uint64_t got;
    uint64_t index;
    uint64_t original_received_count;
    uint64_t recovery_received_count;
} rs_error;

typedef enum rs_rate { RS_RATE_DEFAULT = 0, RS_RATE_HIGH = 1, RS_RATE_LOW = 2 } rs_rate;

typedef struct rs_context rs_context;
typedef struct rs_encoder rs_encoder;
typedef struct rs_decoder rs_decoder;
typedef struct rs_encoder_work rs_encoder_work; /* EncoderWork (src/rate/encoder_work.rs) */
typedef struct rs_decoder_work rs_decoder_work; /* DecoderWork (src/rate/decoder_work.rs) */

/* ---- context: one per device; builds and uploads the GF tables once ---- */
rs_status rs_context_create(int device, rs_context **out);
void rs_context_destroy(rs_context *ctx);
const char *rs_last_device_error(void);
const char *rs_version(void);

/* ---- capability / validation (src/rate/rate_default.rs:15-64, src/rate.rs:91-106) ---- */
int rs_supports(rs_rate rate, uint64_t original_count, uint64_t recovery_count);
/* 1 = HighRate, 0 = LowRate, -1 = unsupported */
int rs_use_high_rate(uint64_t original_count, uint64_t recovery_count);
rs_status rs_validate(rs_rate rate, uint64_t original_count, uint64_t recovery_count, uint64_t shard_bytes,
                      rs_error *err);
/* work_count of the encoder / decoder (rate_high.rs:135-141, 308-312; rate_low.rs same) */
uint64_t rs_encoder_work_count(rs_rate rate, uint64_t original_count, uint64_t recovery_count);
uint64_t rs_decoder_work_count(rs_rate rate, uint64_t original_count, uint64_t recovery_count);

/* ---- one-shot host API (src/lib.rs:251-353) ----
 * rs_encode: `original` = array of original_count pointers to shard_bytes each;
 *   recovery_out = recovery_count * shard_bytes contiguous.
 * rs_decode: original/recovery = arrays of (index, pointer) given as parallel
 *   arrays; restored_out = original_count * shard_bytes, only missing rows
 *   written; restored_mask (original_count bytes) set to 1 for restored rows. */
rs_status rs_encode(rs_context *ctx, uint64_t original_count, uint64_t recovery_count, uint64_t shard_bytes,
                    const uint8_t *const *original, uint64_t original_given, uint8_t *recovery_out, rs_error *err);
rs_status rs_decode(rs_context *ctx, uint64_t original_count, uint64_t recovery_count, uint64_t shard_bytes,
                    const uint64_t *original_index, const uint8_t *const *original, uint64_t original_given,
                    const uint64_t *recovery_index, const uint8_t *const *recovery, uint64_t recovery_given,
                    uint8_t *restored_out, uint8_t *restored_mask, rs_error *err);

/* ---- ReedSolomonEncoder / RateEncoder (src/reed_solomon.rs, src/rate.rs:113-173) ---- */
rs_status rs_encoder_new(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                         uint64_t shard_bytes, rs_encoder **out, rs_error *err);
rs_status rs_encoder_reset(rs_encoder *enc, uint64_t original_count, uint64_t recovery_count,
                           uint64_t shard_bytes, rs_error *err);
rs_status rs_encoder_add_original_shard(rs_encoder *enc, const uint8_t *shard, uint64_t len, rs_error *err);
rs_status rs_encoder_encode(rs_encoder *enc, rs_error *err);
/* valid after a successful encode until rs_encoder_result_drop / next mutation;
 * NULL when index >= recovery_count (src/rate/encoder_work.rs:90-96) */
const uint8_t *rs_encoder_recovery(rs_encoder *enc, uint64_t index);
void rs_encoder_result_drop(rs_encoder *enc); /* EncoderResult::drop -> reset_received */
int rs_encoder_is_high_rate(const rs_encoder *enc);
void rs_encoder_free(rs_encoder *enc);
/* RateEncoder::into_parts (src/rate.rs:129-131): consumes enc (freed), returns its engine
 * (the context) and its working space (host and device buffers) for reuse by another
 * encoder of any rate and shape.  Either out pointer may be NULL.  The work remembers
 * the device of the context it came from: handed to a context on another device, its
 * device buffers are freed (not reused) and only its host buffers are kept. */
rs_status rs_encoder_into_parts(rs_encoder *enc, rs_context **ctx_out, rs_encoder_work **work_out);
/* RateEncoder::new with `work: Option<EncoderWork>` (src/rate.rs:133-139,
 * src/rate/rate_high.rs:93-103): like
 * rs_encoder_new, reusing `work`'s buffers (NULL = none).  `work` is consumed in every
 * case, also when the call fails (as when the reference's new returns Err). */
rs_status rs_encoder_new_with_work(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                   uint64_t recovery_count, uint64_t shard_bytes, rs_encoder_work *work,
                                   rs_encoder **out, rs_error *err);
void rs_encoder_work_free(rs_encoder_work *work);

/* ---- ReedSolomonDecoder / RateDecoder (src/reed_solomon.rs, src/rate.rs:179-250) ---- */
rs_status rs_decoder_new(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                         uint64_t shard_bytes, rs_decoder **out, rs_error *err);
rs_status rs_decoder_reset(rs_decoder *dec, uint64_t original_count, uint64_t recovery_count,
                           uint64_t shard_bytes, rs_error *err);
rs_status rs_decoder_add_original_shard(rs_decoder *dec, uint64_t index, const uint8_t *shard, uint64_t len,
                                        rs_error *err);
rs_status rs_decoder_add_recovery_shard(rs_decoder *dec, uint64_t index, const uint8_t *shard, uint64_t len,
                                        rs_error *err);
rs_status rs_decoder_decode(rs_decoder *dec, rs_error *err);
/* NULL unless original `index` was missing and has been restored
 * (src/rate/decoder_work.rs:189-197) */
const uint8_t *rs_decoder_restored_original(rs_decoder *dec, uint64_t index);
uint64_t rs_decoder_restored_count(const rs_decoder *dec);
void rs_decoder_result_drop(rs_decoder *dec); /* DecoderResult::drop -> reset_received */
int rs_decoder_is_high_rate(const rs_decoder *dec);
void rs_decoder_free(rs_decoder *dec);
/* RateDecoder::into_parts / new with work (src/rate.rs:206-218, src/rate/rate_high.rs:260-270):
 * as for the encoder. */
rs_status rs_decoder_into_parts(rs_decoder *dec, rs_context **ctx_out, rs_decoder_work **work_out);
rs_status rs_decoder_new_with_work(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                   uint64_t recovery_count, uint64_t shard_bytes, rs_decoder_work *work,
                                   rs_decoder **out, rs_error *err);
void rs_decoder_work_free(rs_decoder_work *work);

/* ---- device-resident batch path (HBM in, HBM out) ----
 * d_original: original_count rows, d_recovery: recovery_count rows, both
 * row-major with row stride shard_bytes.  shard_bytes: any positive even
 * size (Error::InvalidShardSize otherwise); whole 64-byte blocks use the
 * reference's block layout (algorithm.md:18-31) and the last S % 64 bytes its
 * tail layout (S % 64 / 2 low bytes, then the high bytes: src/engine/shards.rs:38-74),
 * so shards are byte-identical to the reference's Encoder / Decoder output.
 * Asynchronous on `stream` (device scratch per context and stream: see
 * "Thread-safety" above). */
rs_status rs_encode_device(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                           uint64_t shard_bytes, const void *d_original, void *d_recovery, void *stream,
                           rs_error *err);
/* original_present / recovery_present: HOST arrays of 0/1 bytes.
 * d_restored: original_count rows; only missing originals are written.
 * Missing rows of d_original / d_recovery are never read. */
rs_status rs_decode_device(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                           uint64_t shard_bytes, const void *d_original, const uint8_t *original_present,
                           const void *d_recovery, const uint8_t *recovery_present, void *d_restored, void *stream,
                           rs_error *err);
/* Column slices of wider matrices: shard r of a matrix starts at base + r * stride
 * (stride 0 = shard_bytes; otherwise >= shard_bytes).  Any alignment works:
 * when a base address or stride is not a multiple of 4 the kernels access the
 * caller's matrices byte by byte (slower).  Every engine op is column-wise
 * (src/engine/utils.rs:35-43), so encoding a range of whole 64-byte blocks of
 * each shard yields exactly those blocks of the full recovery shards: the
 * building block of the column-partitioned multi-GPU encode. */
rs_status rs_encode_device_strided(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                   uint64_t shard_bytes, const void *d_original, uint64_t original_stride,
                                   void *d_recovery, uint64_t recovery_stride, void *stream, rs_error *err);
rs_status rs_decode_device_strided(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                   uint64_t shard_bytes, const void *d_original, uint64_t original_stride,
                                   const uint8_t *original_present, const void *d_recovery, uint64_t recovery_stride,
                                   const uint8_t *recovery_present, void *d_restored, uint64_t restored_stride,
                                   void *stream, rs_error *err);
/* A batch of `stripes` independent stripes of one shape (MI355X extension: a
 * storage node codes many stripes at once).  Stripe b's original matrix starts
 * at d_original + b * original_stripe_stride bytes (0 = original_count rows of
 * the row stride), likewise for the recovery / restored matrices; row strides
 * as in the _strided calls.  Where one stripe runs as a single column-kernel
 * launch the whole batch is one launch (stripes x shard_bytes / 8 workgroups);
 * otherwise the stripes run one after another.  Result: identical to
 * `stripes` separate calls.  The decode applies ONE erasure pattern to every
 * stripe (a failed device loses the same shard indices in all of them). */
rs_status rs_encode_device_batch(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                 uint64_t shard_bytes, uint64_t stripes, const void *d_original,
                                 uint64_t original_stride, uint64_t original_stripe_stride, void *d_recovery,
                                 uint64_t recovery_stride, uint64_t recovery_stripe_stride, void *stream,
                                 rs_error *err);
rs_status rs_decode_device_batch(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                 uint64_t shard_bytes, uint64_t stripes, const void *d_original,
                                 uint64_t original_stride, uint64_t original_stripe_stride,
                                 const uint8_t *original_present, const void *d_recovery, uint64_t recovery_stride,
                                 uint64_t recovery_stripe_stride, const uint8_t *recovery_present, void *d_restored,
                                 uint64_t restored_stride, uint64_t restored_stripe_stride, void *stream,
                                 rs_error *err);
/* The batch decode with one erasure pattern PER STRIPE (a receiver doing FEC
 * loses different packets in every block; a repair finds different shards
 * missing in every object).  Matrices, strides and alignment rules are those of
 * rs_decode_device_batch; original_present / recovery_present are HOST arrays of
 * stripes x original_count / stripes x recovery_count bytes of 0/1, stripe-major
 * (row b = stripe b's pattern).
 *   Result: stripe b ends up exactly as if rs_decode_device_strided had been
 * called on it with row b of the two masks: only its missing originals are
 * written, absent input rows are never read, and a stripe with no missing
 * original does no work and writes nothing.
 *   Errors: argument checks first, in rs_decode_device_batch's order (null
 * context / pointers -> RS_ERR_INVALID_ARGUMENT, then rs_validate, then the
 * strides); stripes == 0 -> RS_OK.  Then every stripe's pattern is checked on
 * the host, in stripe order, before any device work; a stripe with fewer than
 * original_count shards in total cannot be decoded (NotEnoughShards).
 *   stripe_status == NULL: all or nothing.  The first such stripe's error is
 *     returned, with that stripe's original_received_count /
 *     recovery_received_count and the stripe's number in err->index (an
 *     extension: the reference's NotEnoughShards has no index); nothing is
 *     launched and nothing is written.
 *   stripe_status != NULL (HOST, stripes bytes): filled with one rs_status per
 *     stripe (RS_OK also for stripes with nothing missing).  Stripes that cannot
 *     be decoded are skipped -- their matrices are neither read nor written --
 *     the others are decoded, and the call returns RS_OK.
 *   Where rs_decode_device_batch runs a batch as one launch (decodes of up to
 * 2^11 work rows on the column kernel) so does this call: the patterns travel
 * to the device as per-stripe descriptors, copied on `stream` ahead of the
 * launch (DESIGN.md "Batches of stripes").  Elsewhere the stripes decode one
 * after another, each with its pattern.  Asynchronous on `stream`; scratch per
 * (context, stream) like every device entry point. */
rs_status rs_decode_device_batch_masks(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                       uint64_t recovery_count, uint64_t shard_bytes, uint64_t stripes,
                                       const void *d_original, uint64_t original_stride,
                                       uint64_t original_stripe_stride, const uint8_t *original_present,
                                       const void *d_recovery, uint64_t recovery_stride,
                                       uint64_t recovery_stripe_stride, const uint8_t *recovery_present,
                                       void *d_restored, uint64_t restored_stride, uint64_t restored_stripe_stride,
                                       uint8_t *stripe_status, void *stream, rs_error *err);

/* ---- repair: the whole stripe back, recovery shards included ----
 * (MI355X extension: a node that lost a disk has lost recovery shards too, and
 * the stripe stays degraded until they are rebuilt.)  A decode that also
 * restores the missing RECOVERY shards, in about the time of the decode: after
 * the decode's last FFT every erased position of the codeword holds its value
 * times the error locator, the recovery positions included, so the reveal
 * multiply that restores an original restores a recovery shard as well
 * (DESIGN.md "Repair") -- no second transform, no gather, no scratch matrix.
 *   Arguments: those of the matching rs_decode_device* call, plus d_recovery_out
 * (recovery_count rows; row / stripe strides as for the other matrices, 0 =
 * shard_bytes / recovery_count rows) between d_restored... and stream.
 *   Contract: missing originals are written to d_restored exactly as by the
 * decode call; missing recovery shard i is written to row i of d_recovery_out,
 * byte-identical to the encoder's recovery shard (block and tail layout of
 * rs_encode_device).  Present rows of either output are never written, absent
 * rows of either input never read.  Unaligned bases or strides take the
 * byte-wise path, as everywhere.
 *   In place: d_recovery_out may be d_recovery (same stride) and d_restored may
 * be d_original -- the natural way to heal a stripe: the holes are filled,
 * nothing else moves.  Safe by construction: the rows written are exactly the
 * rows never read.
 *   Errors, all before any device work, in rs_decode_device_strided's order:
 * null context / pointers (d_recovery_out included) -> RS_ERR_INVALID_ARGUMENT,
 * then rs_validate, then the strides, then NotEnoughShards with its counts
 * (fewer than original_count shards present in total).
 *   Unlike the decode the call does not return early when no original is
 * missing: missing recovery shards alone are rebuilt.  When they form one run
 * of consecutive rows the call runs the encode with its destination narrowed
 * to that run (measured about twice as fast as the decode's kernels there:
 * DESIGN.md "Repair"); any other pattern takes the decode's kernels.  Either
 * way only missing rows are written.  With nothing missing at all it returns
 * RS_OK, launches nothing and writes nothing.  With no recovery shard missing
 * it is the decode call, launch for launch.
 *   rs_repair_device_batch applies ONE pattern to every stripe, like
 * rs_decode_device_batch, and runs as one launch where that call does.
 * Asynchronous on `stream`; scratch per (context, stream); profile records as
 * the decode's, the bytes of a launch counting the recovery rows it writes.
 *   Not covered yet (each can follow now that the kernels take a second
 * destination): the host-memory pipeline (rs_decode_host), the rs_decoder
 * object API and the sharded multi-device decoder.  Per-stripe patterns:
 * rs_repair_device_batch_masks, below. */
rs_status rs_repair_device(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                           uint64_t shard_bytes, const void *d_original, const uint8_t *original_present,
                           const void *d_recovery, const uint8_t *recovery_present, void *d_restored,
                           void *d_recovery_out, void *stream, rs_error *err);
rs_status rs_repair_device_strided(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                   uint64_t shard_bytes, const void *d_original, uint64_t original_stride,
                                   const uint8_t *original_present, const void *d_recovery, uint64_t recovery_stride,
                                   const uint8_t *recovery_present, void *d_restored, uint64_t restored_stride,
                                   void *d_recovery_out, uint64_t recovery_out_stride, void *stream, rs_error *err);
rs_status rs_repair_device_batch(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                 uint64_t shard_bytes, uint64_t stripes, const void *d_original,
                                 uint64_t original_stride, uint64_t original_stripe_stride,
                                 const uint8_t *original_present, const void *d_recovery, uint64_t recovery_stride,
                                 uint64_t recovery_stripe_stride, const uint8_t *recovery_present, void *d_restored,
                                 uint64_t restored_stride, uint64_t restored_stripe_stride, void *d_recovery_out,
                                 uint64_t recovery_out_stride, uint64_t recovery_out_stripe_stride, void *stream,
                                 rs_error *err);
/* The batch repair with one pattern PER STRIPE (a scrub or rebuild pass over
 * many objects, each of which lost a different mix of original and recovery
 * shards; every hole filled in place).  Matrices, strides and alignment rules are
 * those of rs_repair_device_batch; the masks are HOST arrays of stripes x
 * original_count / stripes x recovery_count bytes, stripe-major, as in
 * rs_decode_device_batch_masks.
 *   Result: stripe b ends up exactly as if rs_repair_device_strided had been
 * called on it with row b of the two masks: only missing rows of either output
 * are written, absent input rows are never read, and a stripe that misses
 * nothing does no work.  In place (d_recovery_out == d_recovery, d_restored ==
 * d_original, equal strides) is allowed as above.  Unaligned bases or strides
 * take the byte-wise path.
 *   Errors, all before any device work: null context / pointers (d_recovery_out
 * included) -> RS_ERR_INVALID_ARGUMENT, then rs_validate, then the four row
 * strides; stripes == 0 -> RS_OK.  Then every stripe's pattern is checked on the
 * host in stripe order.  stripe_status as in rs_decode_device_batch_masks: NULL =
 * all or nothing (the first undecodable stripe's NotEnoughShards counts, its
 * number in err->index, nothing launched or written); non-NULL = one rs_status
 * per stripe, undecodable stripes skipped and flagged, the rest repaired, RS_OK.
 * A batch in which no stripe misses anything returns RS_OK, launches nothing and
 * does not touch the context.
 *   Where rs_repair_device_batch runs a batch as one launch (up to 2^11 work
 * rows on the column kernel) so does this call: one launch of
 * k_mono_repair_masks per 65535 stripes, the patterns as per-stripe descriptors
 * copied on `stream` ahead of it.  That launch also takes the stripes that miss
 * recovery shards only through the decode's kernels: a lone rs_repair_device
 * call sends a single run of them to the narrowed encode (7.5 vs 15.3 us at
 * 1024:1024 x 1 KiB), but a batch is heterogeneous and a second launch costs
 * more than it saves.  Elsewhere the stripes run one after another, each by
 * the route rs_repair_device_strided takes for its pattern (the narrowed encode
 * included).
 *   Measured (tools/repair_masks_time.py, profiles/repair_masks/): 64 stripes of
 * 1024:1024 x 1 KiB, each with its own random 1 % of the 2048 shards lost:
 * 64 rs_repair_device calls 1083 us, this call 618 us (0.57), rs_repair_device_batch
 * with one shared pattern 556 us (1.11), rs_decode_device_batch_masks on the same
 * masks, originals only, 580 us (1.07). */
rs_status rs_repair_device_batch_masks(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                       uint64_t recovery_count, uint64_t shard_bytes, uint64_t stripes,
                                       const void *d_original, uint64_t original_stride,
                                       uint64_t original_stripe_stride, const uint8_t *original_present,
                                       const void *d_recovery, uint64_t recovery_stride,
                                       uint64_t recovery_stripe_stride, const uint8_t *recovery_present,
                                       void *d_restored, uint64_t restored_stride, uint64_t restored_stripe_stride,
                                       void *d_recovery_out, uint64_t recovery_out_stride,
                                       uint64_t recovery_out_stripe_stride, uint8_t *stripe_status, void *stream,
                                       rs_error *err);

/* ---- update: a partial-stripe write applied to the recovery shards ----
 * The caller overwrites `count` of the original shards (usually one) and the
 * recovery shards must follow, without the other originals on the device: a
 * parity node holds a few recovery rows and receives the delta of the changed
 * original.  The encode is GF(2^16)-linear per column, so
 *   recovery_j(new) = recovery_j(old) ^ XOR_c G[j][index[c]] * (old_c ^ new_c)
 * with G[j][i] = element j of the encoder's output for the unit stripe (original
 * i = the element 1, every other original zero).
 *   index: HOST array of `count` original indices; row c of d_old and of d_new
 * (count rows of shard_bytes each) is the old / the new content of original
 * index[c].  d_old == NULL: d_new already holds the deltas old ^ new.
 *   d_recovery: recovery_count rows, updated in place (read, XOR, write).
 * recovery_update: HOST mask of recovery_count bytes of 0/1, NULL = every row;
 * rows marked 0 are neither read nor written (their memory need not exist
 * beyond the address arithmetic).  d_old and d_new must NOT overlap d_recovery.
 *   Strides (0 = shard_bytes), alignment and the byte-wise path as in the
 * _strided calls; any even shard_bytes, block and tail layout of
 * rs_encode_device.  rs_update_device_batch applies ONE index list and ONE
 * mask to every stripe (stripe strides 0 = count / recovery_count rows), as
 * rs_repair_device_batch does.  Asynchronous on `stream`, scratch per
 * (context, stream).
 *   Result: the selected recovery rows are byte-identical to rs_encode_device
 * on the stripe with the `count` originals replaced; nothing else is written.
 *   Errors, all before any device work, in this order: null context, d_new,
 * d_recovery, or index with count > 0 -> RS_ERR_INVALID_ARGUMENT; rs_validate;
 * the row strides; then the index list in order: index[c] >= original_count ->
 * InvalidOriginalShardIndex (original_count, index), a repeated index ->
 * DuplicateOriginalShardIndex (index).  count == 0, stripes == 0 or a mask that
 * selects no row: RS_OK, nothing launched, the context not touched.
 *   Routes.  count <= direct_max: one launch of k_update, which forms the deltas
 * once per workgroup and multiplies them into every selected recovery row by
 * the table of log G[j][c]; a batch is the same launch with the stripe as a
 * grid dimension.  The table is built by the first call with a given (rate,
 * original_count, recovery_count, index list) on a stream -- the encode of the
 * unit stripe, 64 * ceil(count / 32) bytes per shard, by whatever route the
 * shape takes -- and kept until another key arrives on that stream or
 * rs_release_stream_scratch frees it; it depends neither on the data nor on
 * the mask.  count > direct_max (and any count > 256): the delta stripe is
 * built in zeroed scratch, encoded, and the selected rows XORed into
 * d_recovery; the stripes of a batch run one after another.
 *   rs_update_set_direct_max sets direct_max for the context (0 = always
 * re-encode); RS_MI355X_UPDATE_DIRECT_MAX does the same at context creation.
 *   Measured (tools/update_time.py, profiles/update/update_time.txt; 1024:1024,
 * delta form, every recovery row, us per call; cold = a new index list every
 * call, so the coefficient step is paid; encode = rs_encode_device on the full
 * stripe, which a caller without all the originals cannot run):
 *     shard   count   direct cold   direct warm   re-encode   encode
 *     1 KiB       1          26.3          12.3        17.9     10.8
 *     1 KiB       8          27.3          11.9        16.5     10.8
 *     1 KiB      16          29.3          11.2        19.1     10.7
 *     1 KiB      32          34.2          12.9        16.8     10.5
 *     1 KiB      64          44.0          22.3        16.6     10.9
 *    64 KiB       1          55.5          33.1       149.9     98.9
 *    64 KiB       8          99.8          79.2       150.4     97.8
 *    64 KiB      16         159.9         139.5       152.0     98.3
 *    64 KiB      32         359.0         338.6       153.2     98.2
 *    64 KiB      64         682.9         662.1       153.5     98.4
 * 64-stripe batch, 1 KiB, count 1: direct 32.3, re-encode 971, batch encode 224.
 * The default direct_max, 16, is the largest measured count at which the warm
 * direct route is still the faster of the two routes at both shard sizes; from
 * count 16 on at 64 KiB it costs more than the full encode.  The whole table
 * and what it says: DESIGN.md "Update". */
#define RS_UPDATE_DIRECT_MAX_DEFAULT 16
rs_status rs_update_device(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                           uint64_t shard_bytes, const uint64_t *index, uint64_t count, const void *d_old,
                           uint64_t old_stride, const void *d_new, uint64_t new_stride, void *d_recovery,
                           uint64_t recovery_stride, const uint8_t *recovery_update, void *stream, rs_error *err);
rs_status rs_update_device_batch(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                 uint64_t shard_bytes, uint64_t stripes, const uint64_t *index, uint64_t count,
                                 const void *d_old, uint64_t old_stride, uint64_t old_stripe_stride,
                                 const void *d_new, uint64_t new_stride, uint64_t new_stripe_stride,
                                 void *d_recovery, uint64_t recovery_stride, uint64_t recovery_stripe_stride,
                                 const uint8_t *recovery_update, void *stream, rs_error *err);
rs_status rs_update_set_direct_max(rs_context *ctx, uint32_t k);

/* ---- update, one index list per stripe ----
 * A batch of partial-stripe writes: every stripe overwrites its OWN originals and
 * takes its OWN recovery-row mask, as the _masks calls of the decode, the repair,
 * the verify, the locate and the heal do.
 *   index: HOST array of stripes x max_count original indices, stripe-major;
 * count: HOST array of `stripes` values, each <= max_count.  Stripe b overwrites
 * originals index[b * max_count + c], c < count[b]; row c of stripe b of d_old /
 * d_new is the old / new content of that original (d_old == NULL: d_new holds the
 * deltas).  Rows c >= count[b] of a stripe's d_old / d_new are never read.  Stripe
 * strides of 0 mean max_count rows for d_old / d_new and recovery_count rows for
 * d_recovery.
 *   recovery_update: NULL (every row of every stripe) or a HOST array of stripes x
 * recovery_count bytes of 0/1, stripe-major: one mask per stripe.  Rows a stripe's
 * mask marks 0 are neither read nor written in that stripe.
 *   Row strides, alignment, the byte-wise path, the block and tail layout, no
 * overlap of d_old / d_new with d_recovery: as in the shared-list batch call above.
 * Asynchronous on `stream`, scratch per (context, stream).  The lists, the counts
 * and the masks may be reused or freed as soon as the call returns: they travel
 * through the stream's pinned staging (which waits for the copy that last read it)
 * and their device copy is reused in stream order.
 *   Result: stripe b ends exactly as if rs_update_device had been called on it with
 * its own list and its own mask row.  A stripe with count[b] == 0, or whose mask
 * selects nothing, is neither read nor written.  The call is all or nothing; there
 * is no status array.
 *   Errors, all before any device work, in this order:
 *   1. null context, d_new or d_recovery, null count with stripes > 0, null index
 *      with stripes > 0 and max_count > 0 -> RS_ERR_INVALID_ARGUMENT;
 *   2. rs_validate;
 *   3. the row strides -> RS_ERR_INVALID_ARGUMENT;
 *   4. stripes == 0 or max_count == 0: RS_OK;
 *   5. every stripe's list, in stripe order, the first offender decides, and
 *      err->got carries the stripe's number (an extension, like err->index of the
 *      _masks calls): count[b] > max_count -> RS_ERR_INVALID_ARGUMENT; an index >=
 *      original_count -> InvalidOriginalShardIndex (original_count, index); an index
 *      repeated within the stripe -> DuplicateOriginalShardIndex (index).  The same
 *      index in two stripes is fine;
 *   6. every count 0, or no stripe with a list selects a row: RS_OK, nothing
 *      launched, the context not touched.
 *   Routes.  Where original_count <= RS_LOCATE_MAX_ORIGINALS and original_count x
 * recovery_count <= RS_LOCATE_MAX_COEFFICIENTS, every stripe with count[b] <=
 * min(direct_max, 256) goes into ONE launch of k_update_lists per 65535 stripes.  Its
 * coefficients are the locate's table of log G[j][i] over every original, the same
 * object: built by the stream's first locate OR first such update of a (rate,
 * original_count, recovery_count) and kept as the locate keeps it, so no index list
 * costs a coefficient step.  The per-list table of rs_update_device is not touched.
 * max_count is only the pitch of `index` and the default stripe stride of d_old /
 * d_new: the lists are staged at the pitch of the longest launched one.
 * Every other stripe (count[b] > direct_max, a shape beyond the bound, every stripe
 * with direct_max == 0) carries count 0 in that launch and then runs on its own,
 * one stripe after another, by whatever route rs_update_device takes for its list
 * and mask row: THAT path pays the coefficient step (or the re-encode) per stripe.
 *   Measured (tools/update_lists_time.py, profiles/update_lists/update_lists_time.txt;
 * 1024:1024, delta form, every recovery row, k random indices per stripe that differ
 * between stripes, us per call; shared = the shared-list batch call with stripe 0's
 * list, which computes something else; loop = one rs_update_device per stripe):
 *     batch          k   this call warm   shared    loop   this call cold
 *     64 x 1 KiB     1             51.5     35.0    1722              508
 *     64 x 1 KiB     8            108.8     79.1    1905              600
 *      1 x 64 KiB    1             54.0     34.7    33.2              510
 *      1 x 64 KiB    8            133.0     80.9    78.3              601
 * 17-33 times faster than the loop for the 64-stripe batch, but 38-64 % slower than
 * the shared-list call where that is an option: k_update_lists takes 48-129 us where
 * k_update takes 35-85 (its logs lie a table row apart).  For a single stripe use
 * rs_update_device.  The whole account: DESIGN.md "Update", an index list per stripe. */
rs_status rs_update_device_batch_lists(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                       uint64_t recovery_count, uint64_t shard_bytes, uint64_t stripes,
                                       const uint64_t *index, const uint32_t *count, uint64_t max_count,
                                       const void *d_old, uint64_t old_stride, uint64_t old_stripe_stride,
                                       const void *d_new, uint64_t new_stride, uint64_t new_stripe_stride,
                                       void *d_recovery, uint64_t recovery_stride, uint64_t recovery_stripe_stride,
                                       const uint8_t *recovery_update, void *stream, rs_error *err);

/* ---- verify: do the recovery shards still agree with the originals? ----
 * The first step of a scrub.  Silent corruption (a flipped bit on a disk or in a
 * buffer) is not an erasure, so rs_repair_device* cannot see it; this call finds
 * the recovery rows to hand to it as absent.
 *   d_original: original_count rows, all present.  d_recovery: recovery_count
 * rows.  recovery_check: HOST mask of recovery_count bytes of 0/1, NULL = every
 * row; rows marked 0 are never read (a degraded stripe is checked on the recovery
 * rows it still has; the memory of the others need not exist beyond the address
 * arithmetic).  d_mismatch: DEVICE array of recovery_count bytes
 * (rs_verify_device_batch: stripes x recovery_count, stripe-major, dense).
 *   Result: after the call every byte of d_mismatch is defined.  Byte
 * b * recovery_count + j is 1 if row j is selected and recovery shard j of stripe
 * b differs, in any of its shard_bytes bytes, from what rs_encode_device would
 * produce from that stripe's originals (block and tail layout of the encode); 0
 * if the row matches and 0 if it is not selected.  Nothing else is written: not
 * the originals, not the recovery shards, not a byte past stripes x
 * recovery_count of the flags.  Bytes between shard_bytes and the row stride are
 * never compared.
 *   Strides (0 = shard_bytes / count rows), alignment and the byte-wise path for
 * unaligned bases or strides as in the _strided / _batch calls.
 * rs_verify_device_batch applies ONE mask to every stripe, as
 * rs_update_device_batch does (a mask per stripe:
 * rs_verify_device_batch_masks below).  Asynchronous on `stream`, scratch per (context,
 * stream).
 *   Errors, all before any device work, in this order: null context, d_original,
 * d_recovery or d_mismatch -> RS_ERR_INVALID_ARGUMENT; rs_validate; the two row
 * strides.  stripes == 0: RS_OK, nothing launched or written, the context not
 * touched.  A mask that selects no row: RS_OK, no kernel, no workspace, the
 * context not touched -- the flags are zeroed by one hipMemsetAsync on `stream`
 * (stripes x recovery_count bytes), so they are defined after this call too; if
 * that memset fails the call returns RS_ERR_DEVICE.
 *   Routes.  Every call first zeroes the flags on `stream`; the kernels store
 * only the ones (plain byte stores of the same value, no atomics).
 *   Fused (k_mono_verify): where the encode is the staged single-chunk column
 * kernel (2^7..2^11 transform rows, at most 256 packs, either rate, 2- and
 * 4-element packs -- the shapes whose batch encode is one launch) the encode's
 * last step loads the caller's word from the address it would have stored to,
 * compares and flags.  One launch per 65535 stripes, no scratch matrix.  With a
 * mask the destination map is narrowed to the span of the selected rows and a
 * selection array, kept with the stream's scratch and copied on `stream` only
 * when the mask changes, says which rows inside the span are compared.  The
 * lane and quad encode kernels have no verify form: the column kernel runs in
 * their place.
 *   Unfused (every shape the encode supports): the encode of the selected span
 * into per-stream scratch (recovery_count rows per stripe: the whole batch where
 * the batch encode is one launch, else stripe by stripe), then k_verify_rows
 * compares scratch and caller rows over the row list.
 *   rs_verify_set_fused: 0 = never fused, 1 = fused where available;
 * RS_MI355X_VERIFY_FUSED does the same at context creation.
 *   Measured (tools/verify_time.py, profiles/verify/verify_time.txt; 1024:1024,
 * every row, us per call; encode = rs_encode_device[_batch] of the same shape,
 * whose kernels are the parent commit's instruction for instruction -- the leg
 * run on the parent's build read 8.38 / 224.4 / 102.1; spread = max - min of the
 * encode leg's five rounds):
 *     shape                 fused   unfused   encode   spread   fused/encode
 *     1 KiB, one stripe     10.65     13.05     8.88     0.57   1.20 (+1.77 us)
 *     1 KiB, 64 stripes     241.2     254.4    223.9     1.73   1.08 (+17.2 us)
 *     64 KiB, one stripe       --     124.3     97.9     7.19   (unfused 1.27)
 * The fused verify was expected to land within the encode's spread; it is
 * outside it, by 1.2 us at one stripe (the memset of the flags is a dispatch of
 * its own) and by 15.5 us over 64 stripes (a load must come back where a store
 * need not: the kernel is 7 % slower than the encode's).  It is no slower than
 * the unfused route at either shape (0.82, 0.95) and needs no scratch matrix,
 * so the default is 1.  DESIGN.md "Verify" has the rest. */
#define RS_VERIFY_FUSED_DEFAULT 1
rs_status rs_verify_device(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                           uint64_t shard_bytes, const void *d_original, uint64_t original_stride,
                           const void *d_recovery, uint64_t recovery_stride, const uint8_t *recovery_check,
                           uint8_t *d_mismatch, void *stream, rs_error *err);
rs_status rs_verify_device_batch(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                 uint64_t shard_bytes, uint64_t stripes, const void *d_original,
                                 uint64_t original_stride, uint64_t original_stripe_stride, const void *d_recovery,
                                 uint64_t recovery_stride, uint64_t recovery_stripe_stride,
                                 const uint8_t *recovery_check, uint8_t *d_mismatch, void *stream, rs_error *err);
rs_status rs_verify_set_fused(rs_context *ctx, int mode);

/* ---- verify with a mask per stripe ----
 * rs_verify_device_batch with recovery_check a HOST array of stripes x
 * recovery_count bytes of 0/1, stripe-major, NOT NULL: row b of it is stripe b's
 * mask.  A scrub runs over many objects and each has lost a different set of
 * recovery rows; this is the batch form that neither reads rows that do not exist
 * nor falls back to one launch per stripe.  Matrices, strides, alignment, the
 * byte-wise path, the block and tail layout and d_mismatch (stripes x
 * recovery_count, dense) are those of rs_verify_device_batch.
 *   Result: stripe b ends exactly as if rs_verify_device had been called on it with
 * row b of the mask.  Every byte of d_mismatch is defined after the call.  A row
 * that stripe b's mask does not select is never read in that stripe -- no prefetch,
 * no load whose result is discarded -- and its memory need not exist beyond the
 * address arithmetic.  Row padding is never compared.  Nothing but the flags is
 * written.  A stripe whose mask selects nothing gets all-zero flags and none of its
 * memory is read.
 *   Asynchronous on `stream`, scratch per (context, stream).  The masks may be
 * reused or freed as soon as the call returns: they are copied through the
 * stream's pinned staging, as the per-stripe descriptors of
 * rs_decode_device_batch_masks are.  The staging waits for the copy that last read
 * it and the device copy is reused in stream order, so two calls in flight on one
 * stream do not overwrite each other's masks.
 *   Errors, all before any device work, in this order: null context, d_original,
 * d_recovery, d_mismatch or recovery_check -> RS_ERR_INVALID_ARGUMENT; rs_validate;
 * the two row strides.  stripes == 0: RS_OK, nothing launched or written, the
 * context not touched.  A batch in which no stripe selects a row: RS_OK, one
 * hipMemsetAsync of the flags on `stream`; no kernel, no workspace, the context not
 * touched.
 *   Routes.  Every call first zeroes the flags on `stream`.  The default is the
 * unfused route (RS_VERIFY_MASKS_FUSED_DEFAULT, measured below); rs_verify_set_fused
 * and RS_MI355X_VERIFY_FUSED set this call's route together with
 * rs_verify_device_batch's.
 *   Fused (k_mono_verify_masks; the shapes of k_mono_verify): one launch per 65535
 * stripes.  The destination map covers the union of the stripes' selected spans;
 * the selection bytes are stripe b's, recovery_count apart.  A lane with nothing
 * to compare loads a row and discards it; that row is the stripe's own first
 * selected row (one word per stripe, loaded wave-uniformly), because the union's
 * first row may be unselected in this stripe.  The workgroups of a stripe that
 * selects nothing return before their first row load.
 *   Unfused: every stripe's row list (recovery_count words apiece) and count are
 * staged; where the batch encode is one launch the encode of the union span goes
 * into scratch and k_verify_rows_masks compares (its grid covers the largest
 * count, workgroups past a stripe's count leave at once); elsewhere stripe by
 * stripe, each stripe's own span, stripes that select nothing skipped.
 *   Measured (tools/verify_masks_time.py, profiles/verify_masks/verify_masks_time.txt;
 * 1024:1024, a random 10 % of every stripe's rows unselected, us per call, median of 5
 * rounds of 50 back-to-back calls; shared = rs_verify_device_batch /
 * rs_locate_device_batch with every row selected, whose kernels are the parent
 * commit's instruction for instruction -- the same leg on the parent's build in the
 * same session read 239.60 / 124.95 (verify) and 230.29 / 124.77 (locate); spread =
 * max - min of the shared leg's five rounds):
 *     verify               masks fused  masks unfused  single calls  shared  spread
 *     1 KiB, 64 stripes        270.96         251.52       1288.72   240.68    0.94
 *     64 KiB, one stripe           --         127.20        118.78   120.36    4.26
 *     locate               masks                                     shared  spread
 *     1 KiB, 64 stripes        256.27                                230.13    0.73
 *     64 KiB, one stripe       131.85                                124.40    0.70
 * The fused masks verify was expected within the shared call's spread plus one small
 * copy; it is NOT: +30.3 us.  Its kernel takes 247.9 us (it loads four selection
 * bytes per lane, which the every-row shared call does not) and the staging copy and
 * its two engine hand-overs take most of the rest.  It is also slower than the
 * unfused masks route (251.5 us: the batch encode 196 us, k_verify_rows_masks 29
 * us), so the DEFAULT for this call is the unfused route; rs_verify_set_fused(ctx,
 * 1) and RS_MI355X_VERIFY_FUSED=1 still force the fused kernel.  Both are far below
 * the 64 single calls (4.7x to 5.1x).  DESIGN.md 4.4k has the rest. */
#define RS_VERIFY_MASKS_FUSED_DEFAULT 0
rs_status rs_verify_device_batch_masks(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                       uint64_t recovery_count, uint64_t shard_bytes, uint64_t stripes,
                                       const void *d_original, uint64_t original_stride,
                                       uint64_t original_stripe_stride, const void *d_recovery,
                                       uint64_t recovery_stride, uint64_t recovery_stripe_stride,
                                       const uint8_t *recovery_check, uint8_t *d_mismatch, void *stream,
                                       rs_error *err);

/* ---- locate: which original of a stripe is corrupt? ----
 * rs_verify_device flags the recovery rows that disagree with the originals.
 * When an ORIGINAL has rotted every recovery row is flagged and nothing says
 * which shard to hand to rs_repair_device* as absent.  This call does: it is the
 * verify plus one word per stripe.
 *   The algebra.  Let D_j = recovery_j ^ encode(originals)_j.  If original i alone
 * is wrong by e (one element per column), D_j = G[j][i] * e in every column and
 * for every row j, with G the coefficient matrix of rs_update_device.  In a
 * column where e != 0 the ratio D_j1 / D_j0 of two rows equals G[j1][i] /
 * G[j0][i], and that ratio names i: the code is MDS, so no 2 x 2 minor of G
 * vanishes.
 *   Arguments, strides (0 = dense), alignment rules, the byte-wise path, the
 * block and tail layout, the HOST mask recovery_check (NULL = every row; rows
 * marked 0 are never read; ONE mask for every stripe of a batch) and d_mismatch
 * are those of rs_verify_device[_batch].  d_located: DEVICE array of one int32_t
 * per stripe (4-byte aligned).  Asynchronous on `stream`, scratch per (context,
 * stream).
 *   Result: after the call every byte of d_mismatch and every word of d_located
 * is defined.  d_mismatch is exactly what rs_verify_device_batch writes for the
 * same arguments.  d_located[b] is
 *   RS_LOCATE_CLEAN    no selected row of stripe b differs.
 *   RS_LOCATE_ROWS     at least one selected row differs and at least one agrees.
 *                      A single corrupt original would make every selected row
 *                      differ, so that is ruled out; the flags name the differing
 *                      rows, as after a verify.  NOT proven: that the originals
 *                      are intact.  Two or more corrupt originals can leave some
 *                      recovery row matching by coincidence (their contributions
 *                      cancel in that row).  The coefficients of low positions lie
 *                      in small subfields, so this happens more often than 2^-16
 *                      per row and column: seen at 128:128 and 128:1024 with
 *                      original 0 off by 1 and the last original off by 2 in one
 *                      column.  A row that agrees vouches for no original.
 *   i in [0, original_count)
 *                      every selected row differs, and in every column and for
 *                      every selected row j, D_j = G[j][i] * e for one e per
 *                      column.  With two or more rows selected (the call takes no
 *                      fewer) that i is unique.  Handing original i to
 *                      rs_repair_device* as absent heals the stripe.
 *   RS_LOCATE_UNKNOWN  every selected row differs and no such i exists: two or
 *                      more corrupt originals, an original plus recovery rows,
 *                      every recovery row corrupt, ...
 * The value depends on the stripe's bytes and the mask alone, not on how it is
 * computed.  Nothing is written but d_located (`stripes` words) and the flags.
 *   How far to trust an i.  With c selected rows, up to c - 1 corrupt shards
 * (originals and selected recovery rows alike) are never attributed to a wrong
 * single original: that would need a vanishing c x c minor of [G | I], and an
 * MDS code has none.  With exactly two selected
 * rows, two corrupt originals CAN be attributed to a third.  Select three rows or
 * more where the stripe has them.
 *   Errors, all before any device work, in this order: null context, d_original,
 * d_recovery, d_located or d_mismatch -> RS_ERR_INVALID_ARGUMENT; rs_validate; the
 * two row strides; recovery_count < 2 or a mask that selects fewer than two rows
 * -> RS_ERR_INVALID_ARGUMENT (rs_verify_device is the call for those); a shape
 * beyond the coefficient table's bound, original_count >
 * RS_LOCATE_MAX_ORIGINALS or original_count x recovery_count >
 * RS_LOCATE_MAX_COEFFICIENTS -> RS_ERR_INVALID_ARGUMENT.  stripes == 0: RS_OK,
 * nothing launched or written, the context not touched.
 *   The table.  log G[j][i] for every i, recovery_count x original_count uint16_t
 * (32 MiB at the bound), is built by the first locate of a (rate,
 * original_count, recovery_count) on a stream: the update's coefficient step over
 * slabs of 256 consecutive originals (the unit stripe of the slab, 512 bytes per
 * shard, the library's encode of it, the logs), so its scratch stays at the
 * update's size.  It is kept with the stream's scratch until another shape
 * arrives or rs_release_stream_scratch frees it, and depends on neither the data
 * nor the mask.  The update's own table is a different one and is not disturbed.
 *   Launches, always the unfused verify's: the flags zeroed, the encode of the
 * selected span into per-stream scratch (the whole batch where the batch encode is
 * one launch, else stripe by stripe), k_verify_rows; then k_locate_find, one
 * workgroup per stripe (CLEAN / ROWS from the flags, else the first column where
 * the first selected row differs, the log ratio against the second selected row
 * there, and the search of the two table rows for it), and k_locate_confirm over
 * every selected row and pack (D_j == (D_j0 / G[j0][i]) * G[j][i], the products the
 * engine's own), whose workgroups leave at once for a stripe without a candidate.
 *   Measured (tools/locate_time.py, profiles/locate/locate_time.txt; 1024:1024,
 * every row, us per call; clean = no stripe differs, corrupt = one corrupt
 * original in every stripe, cold = the table rebuilt; encode =
 * rs_encode_device[_batch] of the same shape, whose kernels are the parent
 * commit's instruction for instruction -- the leg run on the parent's build read
 * 8.28 / 201.8 / 102.6; spread = max - min of the encode leg's five rounds; in
 * brackets the ratio to the encode):
 *     shape                clean         corrupt       cold          unfused verify  encode  spread
 *     1 KiB, one stripe    15.78 (2.14)  23.00 (3.12)  73.60 (9.98)  13.55 (1.84)      7.37    0.42
 *     1 KiB, 64 stripes    239.8 (1.19)  265.5 (1.32)  300.5 (1.49)  233.7 (1.16)     201.6    2.33
 *     64 KiB, one stripe   125.9 (1.29)  163.5 (1.68)  190.7 (1.95)  120.6 (1.24)      97.6    0.34
 * A clean call costs the unfused verify plus TWO small launches (+2.2 / +6.1 /
 * +5.3 us), one more than hoped for: the call is asynchronous, so the confirm is
 * launched whether or not a stripe has a candidate.  A corrupt original in every
 * stripe adds 7.2 / 25.7 / 37.6 us: the confirm is one more read of the scratch
 * and the caller's rows, as expected (27 us against k_verify_rows' 31 over 64
 * stripes); the find's candidate path, one workgroup per stripe, adds 4 us at
 * 1 KiB and 14 us at 64 KiB.  The fused verify (10.55 / 240.5 us) stays the
 * cheaper first pass of a scrub that expects no corrupt originals.  DESIGN.md
 * "Locate" has the rest.
 *   Not covered: stripes with missing
 * originals (rs_locate_device_degraded below locates in those); the host
 * pipeline, the object API and the sharded classes; a fused
 * form on k_mono_verify.  (One corrupt original together with corrupt recovery
 * rows: rs_locate_device_robust below.  Writing the correction back:
 * rs_heal_device below.) */
#define RS_LOCATE_CLEAN (-1)
#define RS_LOCATE_ROWS (-2)
#define RS_LOCATE_UNKNOWN (-3)
#define RS_LOCATE_MAX_ORIGINALS 4096u
#define RS_LOCATE_MAX_COEFFICIENTS (1u << 24)
rs_status rs_locate_device(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                           uint64_t shard_bytes, const void *d_original, uint64_t original_stride,
                           const void *d_recovery, uint64_t recovery_stride, const uint8_t *recovery_check,
                           int32_t *d_located, uint8_t *d_mismatch, void *stream, rs_error *err);
rs_status rs_locate_device_batch(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                 uint64_t shard_bytes, uint64_t stripes, const void *d_original,
                                 uint64_t original_stride, uint64_t original_stripe_stride, const void *d_recovery,
                                 uint64_t recovery_stride, uint64_t recovery_stripe_stride,
                                 const uint8_t *recovery_check, int32_t *d_located, uint8_t *d_mismatch, void *stream,
                                 rs_error *err);

/* ---- locate with a mask per stripe ----
 * rs_locate_device_batch with the per-stripe masks of
 * rs_verify_device_batch_masks (HOST, stripes x recovery_count bytes, NOT NULL;
 * copied through the stream's staging, free to reuse when the call returns).
 * Everything else -- matrices, strides, d_mismatch, d_located, the table -- is the
 * plain locate's.  Stripe b ends exactly as if rs_locate_device had been called on
 * it with row b of the mask; a row its mask does not select is never read in that
 * stripe.  Every byte of d_mismatch and every word of d_located is defined after
 * the call; nothing else is written.
 *   Errors, all before any device work, in this order: null context, d_original,
 * d_recovery, d_located, d_mismatch or recovery_check -> RS_ERR_INVALID_ARGUMENT;
 * rs_validate; the two row strides; stripes == 0: RS_OK; recovery_count < 2,
 * original_count > RS_LOCATE_MAX_ORIGINALS or original_count x recovery_count >
 * RS_LOCATE_MAX_COEFFICIENTS -> RS_ERR_INVALID_ARGUMENT.  Then every stripe's mask is
 * counted on the host, in stripe order.  A stripe that selects fewer than two
 * rows cannot be located, and
 *   stripe_status == NULL: the call is all or nothing.  RS_ERR_INVALID_ARGUMENT with
 *     the first such stripe's number in err->index; nothing is launched, nothing
 *     is written.
 *   stripe_status != NULL (HOST, `stripes` bytes): every stripe gets one rs_status,
 *     RS_OK or RS_ERR_INVALID_ARGUMENT.  A stripe that cannot be located is skipped:
 *     none of its rows is read, its flags are all 0 and d_located[b] =
 *     RS_LOCATE_SKIPPED.  The others are located and the call returns RS_OK.
 *   The table is the plain locate's, shared with it both ways: a warm stream builds
 * none for either call.
 *   Launches, per 65535 stripes: the unfused route of
 * rs_verify_device_batch_masks, then k_locate_find_masks (j0, j1 and the count of
 * selected rows are the stripe's; a skipped stripe's workgroup stores
 * RS_LOCATE_SKIPPED and reads nothing of it) and k_locate_confirm_masks (its grid
 * covers the largest count).
 *   Measured (tools/verify_masks_time.py, profiles/verify_masks/): see DESIGN.md
 * §4.4k.
 *   Not covered: per-stripe masks for the robust and the degraded calls (the heal
 * has them: rs_heal_device_batch_masks below); a fused form on k_mono_verify_masks; the host pipeline, the object API
 * and the sharded classes. */
#define RS_LOCATE_SKIPPED (-4)
rs_status rs_locate_device_batch_masks(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                       uint64_t recovery_count, uint64_t shard_bytes, uint64_t stripes,
                                       const void *d_original, uint64_t original_stride,
                                       uint64_t original_stripe_stride, const void *d_recovery,
                                       uint64_t recovery_stride, uint64_t recovery_stripe_stride,
                                       const uint8_t *recovery_check, int32_t *d_located, uint8_t *d_mismatch,
                                       uint8_t *stripe_status, void *stream, rs_error *err);

/* ---- robust locate: one corrupt original among corrupt recovery rows ----
 * rs_locate_device needs every selected recovery row but the damage of the one
 * original to be clean: it takes its candidate from the first two selected rows
 * and gives up on the first row that disagrees, so one corrupt original plus one
 * flipped bit in any recovery row comes back RS_LOCATE_UNKNOWN.  This call
 * tolerates up to max_outliers corrupt selected rows beside the original, and
 * names them.
 *   Arguments: those of rs_locate_device[_batch], in the same order, with
 * max_outliers after recovery_check and d_outlier after d_mismatch.  d_outlier:
 * DEVICE array of stripes x recovery_count bytes, stripe-major and dense, like the
 * flags.  With c = the number of selected rows and t = max_outliers the call
 * requires 2 (1 + t) <= c and t <= RS_LOCATE_MAX_OUTLIERS.
 *   Result: after the call every byte of d_mismatch, every word of d_located and
 * every byte of d_outlier is defined.  d_mismatch is exactly what
 * rs_verify_device_batch writes for the same arguments.  d_located[b] is
 *   RS_LOCATE_CLEAN, RS_LOCATE_ROWS
 *                      exactly as by rs_locate_device: fewer than c selected rows
 *                      differ (with the same "NOT proven").  d_outlier of the
 *                      stripe is all 0.
 *   i in [0, original_count)
 *                      every selected row differs, and there are one e per column
 *                      and a set B of at most t selected rows such that D_j =
 *                      G[j][i] * e in every column for every selected j outside B.
 *                      d_outlier[b][j] = 1 exactly for j in B and 0 elsewhere,
 *                      unselected rows included.  Handing original i and the rows
 *                      of B to rs_repair_device* as absent heals the stripe.
 *   RS_LOCATE_UNKNOWN  every selected row differs and no such (i, e, B) exists.
 *                      d_outlier of the stripe is all 0.
 * Nothing is written but the three outputs.
 *   1. Uniqueness.  Two explanations (i, e, B) and (i', e', B') share at least
 * c - 2t >= 2 selected rows outside B and B'.  If i != i', two such rows j, k give
 * G[j][i] e = G[j][i'] e' and G[k][i] e = G[k][i'] e' in every column; the 2 x 2
 * minor of G on rows j, k and columns i, i' does not vanish (the code is MDS), so
 * e = e' = 0 in every column, and then D_j = 0: row j does not differ, against
 * "every selected row differs".  If i = i', one shared row j gives G[j][i] e =
 * G[j][i] e' with G[j][i] != 0, so e = e', and then B = B' = the selected rows
 * with D_j != G[j][i] e.  So i, e and B are functions of the stripe's bytes, the
 * mask and t alone, not of how they are found.
 *   2. Trust.  Suppose the true damage is s corrupt shards, originals and selected
 * recovery rows alike, with s + 1 + t <= c.  Then the call never names a wrong
 * (i, B).  The originals and the c selected rows are a word of an
 * [original_count + c, original_count] MDS code, of distance c + 1.  The stored
 * word is within s of the true codeword; an answer (i, B) is a codeword (the
 * originals with e taken off original i, and its encode) within 1 + |B| <= 1 + t
 * of the stored word.  Were the two different, they would be two codewords within
 * s + 1 + t <= c of one another, less than the distance.  So the answer's
 * codeword IS the true one: i and B are among the truly corrupt shards.  This
 * replaces rs_locate_device's "c - 1 corrupt shards" statement; at the largest
 * allowed t = c/2 - 1 it is s <= c/2, the unique-decoding radius.
 *   3. Compatibility.  With max_outliers == 0 the results in d_located and
 * d_mismatch are those of rs_locate_device_batch for the same arguments (B is
 * empty: the contract above is the locate's), and d_outlier is all zero.
 *   Errors, all before any device work, in this order: rs_locate_device_batch's
 * checks, with d_outlier among the null-pointer checks; then max_outliers >
 * RS_LOCATE_MAX_OUTLIERS or 2 (1 + max_outliers) > c -> RS_ERR_INVALID_ARGUMENT;
 * then the locate's shape bound.  stripes == 0: RS_OK, nothing launched or
 * written, the context not touched.
 *   How it is found.  Of the first t + 1 disjoint pairs of the selected-row list,
 * (sel[0], sel[1]), (sel[2], sel[3]), ..., one at least has both rows outside B.
 * Each pair p gives a candidate as rs_locate_device's two rows do: the first
 * column where D_sel[2p] != 0, the log ratio against D_sel[2p+1] there, the i with
 * that ratio in the table.  A candidate from a spoiled pair can be wrong, or right
 * in i with a wrong e (its reference row an outlier damaged where e = 0).  So each
 * candidate is confirmed with e from ITS OWN reference row, e = D_sel[2p] /
 * G[sel[2p]][i_p], by counting the selected rows that disagree in any pack; the
 * first candidate with at most t is the answer, and by 1. any that passes names
 * the same (i, e, B).
 *   Launches: the locate's up to k_verify_rows (its coefficient table shared with
 * rs_locate_device and rs_heal_device both ways), d_outlier zeroed beside the
 * flags; then per group of stripes a memset of (t + 1) x recovery_count vote bytes
 * per stripe in per-stream scratch, k_locate_find_pairs (one workgroup per stripe
 * and pair; CLEAN / ROWS from the flags, else the pair's candidate), k_locate_count (the
 * confirm's grid; each row's D_j loaded once and checked against every
 * candidate; a disagreeing lane stores the byte 1 to votes[stripe][p][j]) and
 * k_locate_decide (one workgroup per stripe: the sums, d_located, the d_outlier
 * row).
 *   Measured (tools/locate_robust_time.py,
 * profiles/locate_robust/locate_robust_time.txt; 1024:1024, every row, us per
 * call, the legs interleaved in one session; locate = rs_locate_device_batch,
 * whose kernels are the parent commit's -- the same legs on the parent's build
 * read 22.27 / 240.35 / 126.12 clean and 25.83 / 266.20 / 163.87 corrupt; spread =
 * max - min of its five rounds; original = one corrupt original in every stripe,
 * outlier = the same plus one flipped bit in recovery row 0 of every stripe):
 *     shape               locate clean (spread)  locate original (spread)  t=1 clean / original / outlier  t=7 clean / original / outlier
 *     1 KiB, one stripe    23.64 (10.91)          26.19 (5.44)              29.93 /  34.92 /  34.13         32.32 /  40.06 /  39.74
 *     1 KiB, 64 stripes   242.32 (0.88)          267.43 (0.57)             244.86 / 287.27 / 286.95        247.86 / 324.60 / 321.87
 *     64 KiB, one stripe  123.97 (4.57)          164.07 (0.64)             129.35 / 187.97 / 186.83        130.17 / 215.34 / 213.09
 * A clean batch costs the locate plus about one small launch, as expected: +6.3 /
 * +2.5 / +5.4 us at t = 1, +8.7 / +5.6 / +6.2 at t = 7 (one kernel and two memsets
 * more; the single 1 KiB stripe was bimodal in the session, 15 and 22-26 us).  The
 * damaged case does NOT cost the locate's corrupt case: +8.7 / +19.8 / +23.9 us at
 * t = 1 and +13.9 / +57.2 / +51.3 us at t = 7.  The find costs what the locate's
 * does and the rows are read once; the excess is k_locate_count (39.8 / 47.5 us
 * at t = 1, 78.4 / 73.4 at t = 7 by the events, against k_locate_confirm's 26.0 /
 * 27.9): every workgroup of 16 rows first forms e for each of the t + 1
 * candidates, and the candidate loop inside the row loop keeps loads and products
 * of neighbouring rows from overlapping.  DESIGN.md "Robust locate" has the rest.
 *   rs_heal_device_robust below is this call
 * writing the correction in place (a robust heal).
 *   Not covered: two or more corrupt originals; a mask per stripe; stripes with
 * missing originals (rs_locate_device_degraded below locates in those); the host
 * pipeline, the object API and the sharded classes. */
#define RS_LOCATE_MAX_OUTLIERS 7u
rs_status rs_locate_device_robust(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                  uint64_t shard_bytes, const void *d_original, uint64_t original_stride,
                                  const void *d_recovery, uint64_t recovery_stride, const uint8_t *recovery_check,
                                  uint32_t max_outliers, int32_t *d_located, uint8_t *d_mismatch, uint8_t *d_outlier,
                                  void *stream, rs_error *err);
rs_status rs_locate_device_robust_batch(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                        uint64_t recovery_count, uint64_t shard_bytes, uint64_t stripes,
                                        const void *d_original, uint64_t original_stride,
                                        uint64_t original_stripe_stride, const void *d_recovery,
                                        uint64_t recovery_stride, uint64_t recovery_stripe_stride,
                                        const uint8_t *recovery_check, uint32_t max_outliers, int32_t *d_located,
                                        uint8_t *d_mismatch, uint8_t *d_outlier, void *stream, rs_error *err);

/* ---- degraded locate: the locate of a stripe with missing originals ----
 * The calls above need every original.  With a disk out the caller has only
 * rs_decode_device* / rs_repair_device*, which trust every present shard: one
 * flipped bit in a present original, or in a recovery row the decode uses, is
 * multiplied into every restored original and nothing reports it.  This call is
 * the decode of such a stripe together with the locate's check of it.
 *   The algebra is the locate's.  Any original_count shards of an MDS codeword are
 * an information set.  With m originals missing, the present originals and m
 * reference recovery rows are one; the remaining selected rows are parity over it.
 * One corrupt shard of the set, wrong by e, contributes T[j][p] * e to check row j,
 * with a coefficient matrix T that has no zero entry and no vanishing 2 x 2 minor.
 *   Definitions.  m = the number of missing originals.  sel = the selected rows
 * in increasing order, c = |sel|.  The reference rows are R = sel[0..m), the check
 * rows K = sel[m..c).  F_b = stripe b's originals completed from R: the present
 * rows as stored, the missing rows as rs_decode_device restores them with
 * recovery_present = the indicator of R.  D_j = recovery_j ^ encode(F_b)_j.  The
 * information position of an index p in [0, original_count) is original p where it
 * is present, else reference row R[rank of p among the missing originals].
 *   Arguments.  original_present: HOST mask of original_count bytes, required; ONE
 * mask for every stripe of a batch, as rs_repair_device_batch; absent rows of
 * d_original are never read.  recovery_check: HOST mask, NULL = every row, ONE mask
 * for a batch; unselected rows are never read.  d_restored may be NULL (see below).
 * Strides (0 = dense), alignment rules, the byte-wise path and the block and tail
 * layout are those of the _strided / _batch calls; d_located and d_mismatch those of
 * rs_locate_device[_batch].  Asynchronous on `stream`, scratch per (context, stream).
 *   Result: after the call every byte of d_mismatch and every word of d_located is
 * defined.  d_mismatch[b][j] is 1 exactly for j in K with D_j != 0; it is 0 for
 * reference rows and unselected rows.  d_located[b] is
 *   RS_LOCATE_CLEAN    no row of K differs.
 *   RS_LOCATE_ROWS     some rows of K differ and some agree.  A single corrupt
 *                      information shard would make every row of K differ, so that
 *                      is ruled out; the flags name the differing rows.  NOT proven:
 *                      that the information shards are intact.  Two or more corrupt
 *                      ones can leave some check row matching by coincidence (their
 *                      contributions cancel in that row), as rs_locate_device's
 *                      section describes: a row that agrees vouches for no shard.
 *   i in [0, original_count), original i present
 *                      every row of K differs, and D_j = T[j][i] * e for one e per
 *                      column, over every j in K.  Original i is the corrupt shard.
 *   original_count + j, j in R
 *                      the same statement for the information position that
 *                      reference row j stands in.  Recovery row j is the corrupt shard.
 *   RS_LOCATE_UNKNOWN  every row of K differs and no position explains it.
 * The value depends on the stripe's bytes and the two masks alone, not on how it
 * is computed.
 *   Uniqueness and trust, on the [original_count + |K|, original_count] MDS code
 * that the information shards and the rows of K are a word of.  With |K| >= 2 (the
 * call takes no fewer) a named position is unique: two positions explaining the
 * same D over two rows would need a vanishing 2 x 2 minor of T.  Up to |K| - 1
 * corrupt shards among the original_count information shards and the rows of K are
 * never attributed to a wrong position: that would need a vanishing |K| x |K| minor
 * of [T | I], and an MDS code has none.  With exactly two check rows, two corrupt
 * information shards CAN be attributed to a third.  Select three check rows where
 * the stripe has them.
 *   d_restored.  When it is non-NULL the missing originals' rows receive F_b's
 * missing rows, byte-identical to rs_decode_device_batch with the R mask; present
 * rows are never written.  It may alias d_original with equal strides (the
 * repair's in-place argument: the rows written are exactly the rows never read;
 * the later kernels read the recovery matrix and scratch).  The restored rows are
 * trustworthy on CLEAN, and on ROWS with the caveat above.  After a located or
 * UNKNOWN stripe they were decoded from a corrupt shard: re-run rs_repair_device*
 * with the named shard absent.  Nothing is written but d_located, the flags and
 * those rows.
 *   m == 0: d_located and d_mismatch equal rs_locate_device_batch's for the same
 * arguments, d_restored is untouched; the call delegates to the locate and shares
 * its table.
 *   Errors, all before any device work, in this order: null context, d_original,
 * original_present, d_recovery, d_located or d_mismatch -> RS_ERR_INVALID_ARGUMENT;
 * rs_validate; the row strides (restored_stride when d_restored is given); c < m ->
 * RS_ERR_NOT_ENOUGH_SHARDS with the decode's counts (original_received_count =
 * original_count - m, recovery_received_count = c); c < m + 2 ->
 * RS_ERR_INVALID_ARGUMENT (decodable, but nothing is left to check with); the
 * locate's shape bound.  stripes == 0: RS_OK, nothing launched or written, the
 * context not touched.
 *   Launches per group of stripes (a group: what rs_repair_device_batch runs as one
 * launch; elsewhere one stripe), after the flags are zeroed: the repair with
 * recovery_present = the indicator of R, its restored originals to d_restored or to
 * per-stream scratch and its second output -- every recovery row outside R of the
 * completed stripe, in one decode -- to a per-stream scratch matrix, the locate's
 * `want`: no fill copy and no second encode.  Then k_verify_rows over K,
 * k_locate_find and k_locate_confirm with the row list K and the table T, and
 * k_locate_rename, one thread per stripe, which turns a located index p of a missing
 * original into original_count + R[rank(p)] through an original_count-entry map.
 *   The table.  log T[j][p], recovery_count x original_count uint16_t, every row
 * outside R filled, is built by the first call with a given key on a stream: (rate,
 * original_count, recovery_count, the original_present bytes, R).  Every row a call
 * may check is filled, so the rows of K are not part of the key.  It is built over
 * slabs of 256 positions as the locate's: k_coef_unit_degraded writes the element 1
 * of position p into unit original p or into unit reference row R[rank(p)], the
 * repair above runs on the unit stripe, k_coef_log_slab takes the logs.  It is kept
 * with the stream's scratch until another key arrives or
 * rs_release_stream_scratch frees it, and depends on neither the data nor
 * d_restored.  The locate's table and the update's are different ones and are not
 * disturbed.
 *   Measured (tools/locate_degraded_time.py,
 * profiles/locate_degraded/locate_degraded_time.txt; 1024:1024, every row selected,
 * d_restored = d_original, us per call, median of five rounds of 50 back-to-back
 * calls, the legs interleaved in one session; clean = no stripe differs, corrupt =
 * one corrupt present original in every stripe, cold = the table rebuilt;
 * yardstick = what a caller had before, rs_repair_device_batch with
 * recovery_present = R in place and then rs_locate_device_batch under the mask K,
 * both the parent commit's kernels, on the same clean / corrupt stripes -- where it
 * can only answer UNKNOWN; spread = max - min of the yardstick's five rounds):
 *     shape, m                clean    corrupt  cold     yardstick clean (spread) / corrupt (spread)
 *     1 KiB, one stripe, 1     25.21    31.60   121.38    29.57 (1.93) /  35.19 (1.90)
 *     1 KiB, one stripe, 16    25.53    32.52   124.57    31.37 (1.45) /  36.74 (1.18)
 *     1 KiB, 64 stripes, 1    537.23   566.68   632.44   737.94 (0.96) / 743.27 (1.79)
 *     1 KiB, 64 stripes, 16   557.29   585.47   655.76   754.96 (1.52) / 775.42 (1.62)
 *     64 KiB, one stripe, 1   250.82   288.63   354.43   359.37 (1.22) / 374.87 (1.08)
 *     64 KiB, one stripe, 16  292.35   335.73   401.35   396.53 (0.62) / 414.14 (0.56)
 * The expectation was "the repair of the same pattern plus the locate's three small
 * launches and one more", so within the yardstick's spread plus one launch floor
 * (6.0-6.6 us, the shortest launch of the call by the library's events).  Every case
 * lands within it, and below the yardstick: by 4.4 / 5.8 us on the single 1 KiB
 * stripe, by 201 / 198 us on 64 stripes and by 109 / 104 us at 64 KiB, which is the
 * yardstick's encode (k_mono<10> 10 / 209 us, three passes 111 us by the events) that
 * the repair's second output makes unnecessary, less k_locate_rename (6.0-7.2 us).
 * By the events a clean call is the repair (18.5 / 545 / 233 us at m = 1), k_verify_rows
 * (6.4 / 30.7 / 26.6 us) and three launches at the floor.  A corrupt original in every
 * stripe adds 6.4-7.0 / 28-29 / 38-43 us: the find's candidate path and the confirm, as
 * in the locate.  The cold call adds 95-109 us: four slabs of (k_coef_unit_degraded, a
 * one-stripe repair at 16-18 us, k_coef_log_slab).  A degraded stripe costs far more
 * than a whole one (rs_locate_device_batch: 240 us for 64 clean stripes): the repair
 * from m reference rows writes every other recovery row, where the locate's encode
 * is one transform.  DESIGN.md "Degraded locate" has the rest.
 *   Not covered: writing the correction back (a degraded heal); max_outliers; a
 * mask per stripe; the host pipeline, the object API and the sharded classes.
 * (rs_heal_device_degraded below is that heal.) */
rs_status rs_locate_device_degraded(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                    uint64_t shard_bytes, const void *d_original, uint64_t original_stride,
                                    const uint8_t *original_present, const void *d_recovery, uint64_t recovery_stride,
                                    const uint8_t *recovery_check, void *d_restored, uint64_t restored_stride,
                                    int32_t *d_located, uint8_t *d_mismatch, void *stream, rs_error *err);
rs_status rs_locate_device_degraded_batch(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                          uint64_t recovery_count, uint64_t shard_bytes, uint64_t stripes,
                                          const void *d_original, uint64_t original_stride,
                                          uint64_t original_stripe_stride, const uint8_t *original_present,
                                          const void *d_recovery, uint64_t recovery_stride,
                                          uint64_t recovery_stripe_stride, const uint8_t *recovery_check,
                                          void *d_restored, uint64_t restored_stride, uint64_t restored_stripe_stride,
                                          int32_t *d_located, uint8_t *d_mismatch, void *stream, rs_error *err);

/* ---- heal: fix what the locate found, in place, on the device ----
 * A scrub built from the calls above is three calls with a host round trip in the
 * middle: rs_locate_device_batch, a synchronize and a read of d_located and the
 * flags, then rs_repair_device_batch_masks, a full decode of every damaged stripe.
 * Yet at the end of the locate everything a heal needs is on the device: for a
 * located original i the confirm has just formed e = D_j0 / G[j0][i] (j0: the first
 * selected row) in every column, and the clean shard is original_i ^ e; for a
 * RS_LOCATE_ROWS stripe the clean recovery rows are the encode of the stored
 * originals, still in the per-stream scratch.  This call is the locate followed by
 * one more launch per group of stripes that writes those: asynchronous on
 * `stream`, no host synchronization, no masks per stripe, no decode.
 *   Arguments, strides (0 = dense), alignment rules, the byte-wise path, the block
 * and tail layout and the HOST mask recovery_check (NULL = every row; ONE mask for
 * every stripe) are those of rs_locate_device[_batch]; rows marked 0 are never
 * read and never written.  d_original and d_recovery are written in place.
 * mode: RS_HEAL_ORIGINAL | RS_HEAL_RECOVERY, at least one.  d_action: DEVICE
 * array of one byte per stripe.
 *   Result.  d_located and d_mismatch hold exactly what rs_locate_device_batch
 * writes for the same arguments: they describe the stripe AS FOUND, before
 * anything is healed (a caller logs them).  Every byte of d_action is defined:
 *   RS_HEAL_ORIGINAL  d_located[b] = i >= 0 and mode has the bit: original i of
 *                     stripe b has become original_i ^ e, e = D_j0 / G[j0][i] per
 *                     column.  Only its shard_bytes bytes are written, not the row
 *                     padding.  The confirm has shown D_j = G[j][i] * e for every
 *                     selected row, so every selected row now agrees; and when
 *                     original i alone was corrupt the row is byte-identical to
 *                     the clean shard, since G[j0][i] != 0 makes e unique.
 *   RS_HEAL_RECOVERY  d_located[b] = RS_LOCATE_ROWS, mode has the bit, and at most
 *                     max_rows selected rows differ: each differing selected row
 *                     of d_recovery has become the encode of the stored originals
 *                     (shard_bytes bytes each; rows that agree, unselected rows
 *                     and padding are not written).  max_rows is the caller's
 *                     majority threshold; 0 never rewrites.
 *   0                 the stripe is untouched: CLEAN, UNKNOWN, ROWS above the
 *                     threshold, or an outcome whose mode bit is off.
 * Nothing else is written anywhere.  A second heal of a healed stripe reports
 * RS_LOCATE_CLEAN with action 0.
 *   CAVEAT (the locate's "NOT proven", carried over): a ROWS stripe does not prove
 * the originals intact.  RS_HEAL_RECOVERY can make recovery rows consistent with
 * CORRUPT originals -- after which a verify says clean and the damage can no
 * longer be found.  max_rows and the choice to set the bit belong to the caller:
 * keep max_rows well below half of the selected rows, so that the agreeing rows
 * outvote the rewritten ones.
 *   Errors, all before any device work, in this order: null context, d_original,
 * d_recovery, d_located, d_mismatch or d_action -> RS_ERR_INVALID_ARGUMENT;
 * rs_validate; the two row strides; mode == 0 or a bit outside the two ->
 * RS_ERR_INVALID_ARGUMENT (rs_locate_device is the call for mode 0); fewer than 2
 * selected rows, or fewer than 3 with RS_HEAL_ORIGINAL -> RS_ERR_INVALID_ARGUMENT
 * (with two rows, two corrupt originals can be attributed to a third, see above;
 * this call writes on that evidence, so it takes three); the locate's shape bound.
 * stripes == 0: RS_OK, nothing launched or written, the context not touched.  The
 * matrices must not overlap one another or the three outputs.
 *   Launches: the locate's, group of stripes by group of stripes, its coefficient
 * table shared with it (a locate after a heal on the stream finds the table, and
 * the reverse); k_locate_find also stores each stripe's count of differing rows
 * into per-stream scratch; and one k_heal per group directly after that group's
 * k_locate_confirm, while the group's encode is still in scratch (off the column
 * kernel a group is one stripe and the scratch is reused).  k_heal has the
 * confirm's grid; workgroups of a stripe with nothing to do leave at once.
 *   Measured (tools/heal_time.py, profiles/heal/heal_time.txt; 1024:1024, every
 * row, both mode bits, max_rows 16, us per call, the legs interleaved in one
 * session; locate = rs_locate_device_batch on the clean batch, whose kernels are
 * the parent commit's, spread = max - min of its five rounds; original / row = one
 * corrupt original / one corrupt recovery row in EVERY stripe; scrub = the three
 * calls with their synchronize, host read and masks; the four damaged legs net
 * of the 4.3-4.5 us launch that puts the damage back before each call; in
 * brackets the ratio to the locate):
 *     shape               locate spread  heal clean    heal original heal row      scrub original scrub row
 *     1 KiB, one stripe    15.50   0.77  18.10 (1.17)  21.26 (1.37)  18.71 (1.21)   98.4 (6.35)    89.6 (5.78)
 *     1 KiB, 64 stripes   241.0    1.33  244.0 (1.01)  272.1 (1.13)  247.3 (1.03)  987.4 (4.10)   996.9 (4.14)
 *     64 KiB, one stripe  125.0    5.53  128.6 (1.03)  169.9 (1.36)  132.1 (1.06)  399.7 (3.20)   275.0 (2.20)
 * A clean heal costs the locate plus one small launch, as expected: +2.6 / +3.0 /
 * +3.6 us, k_heal at the 6.1-6.3 us floor between two of the library's events
 * (at the single 1 KiB stripe the leg's own rounds spread 3.3 us, more than the
 * difference).  A healed ROW costs 3.2 / 6.3 / 7.0 us over the locate: k_heal's
 * copy is 8.6-9.2 us by the events.  A healed ORIGINAL costs 5.8 / 31.1 / 44.9 us
 * over the CLEAN locate, but that is the locate's own corrupt case (the find's
 * candidate path and the confirm: +7.2 / +25.7 / +37.6 us when it was measured
 * alone, above) plus the k_heal launch, which stays at 6.4-6.8 us: one row read
 * and written.  Both beat the three-call scrub by more than its decode's time
 * (k_mono_repair_masks 20-22 / 589-617 us, the 64 KiB decode's passes 164 /
 * 103 us by the events): by 77 / 715 / 230 us for an original and 71 / 750 /
 * 143 us for a row, the rest being the synchronize, the two reads on the host and
 * the masks.  DESIGN.md "Heal" has the rest.
 *   Not covered: a mask per stripe; stripes with missing originals
 * (rs_locate_device_degraded above locates in those); the host
 * pipeline, the object API and the sharded classes.  (The mask per stripe is not
 * covered by these two calls: rs_heal_device_batch_masks below takes one.  The
 * robust and the degraded heal have no such form.) */
#define RS_HEAL_ORIGINAL 1u /* a located original i: original_i ^= e */
#define RS_HEAL_RECOVERY 2u /* a ROWS stripe: rewrite its differing selected rows */
rs_status rs_heal_device(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                         uint64_t shard_bytes, void *d_original, uint64_t original_stride, void *d_recovery,
                         uint64_t recovery_stride, const uint8_t *recovery_check, uint32_t mode, uint32_t max_rows,
                         int32_t *d_located, uint8_t *d_mismatch, uint8_t *d_action, void *stream, rs_error *err);
rs_status rs_heal_device_batch(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                               uint64_t shard_bytes, uint64_t stripes, void *d_original, uint64_t original_stride,
                               uint64_t original_stripe_stride, void *d_recovery, uint64_t recovery_stride,
                               uint64_t recovery_stripe_stride, const uint8_t *recovery_check, uint32_t mode,
                               uint32_t max_rows, int32_t *d_located, uint8_t *d_mismatch, uint8_t *d_action,
                               void *stream, rs_error *err);

/* ---- heal with a mask per stripe ----
 * rs_heal_device_batch with the per-stripe masks of rs_locate_device_batch_masks:
 * recovery_check is a HOST array of stripes x recovery_count bytes of 0/1,
 * stripe-major, NOT NULL; it is copied through the stream's staging and may be
 * reused or freed when the call returns.  Everything else -- matrices, strides,
 * mode, max_rows, the three outputs, the table -- is the heal's.
 *   Stripe b ends exactly as if rs_heal_device had been called on it with row b of
 * the mask and the same mode and max_rows: d_located and d_mismatch describe the
 * stripe as found and equal what rs_locate_device_batch_masks writes; d_action[b]
 * and both matrices are as rs_heal_device leaves them (e comes from the STRIPE's
 * first selected row); max_rows is compared with the stripe's own count of
 * differing selected rows.  A row that stripe b's mask does not select is never read
 * and never written in that stripe.  Every byte of d_mismatch and d_action and every
 * word of d_located is defined after the call; row padding, stripe padding and
 * anything else are untouched.  The CAVEAT of rs_heal_device about RS_HEAL_RECOVERY
 * holds here unchanged.
 *   Errors, all before any device work, in this order: null context, d_original,
 * d_recovery, d_located, d_mismatch, d_action or recovery_check ->
 * RS_ERR_INVALID_ARGUMENT; rs_validate; the two row strides; mode == 0 or a bit
 * outside the two -> RS_ERR_INVALID_ARGUMENT; stripes == 0: RS_OK, nothing touched;
 * recovery_count < need (need = 3 with RS_HEAL_ORIGINAL, else 2: the heal's own
 * rule), original_count > RS_LOCATE_MAX_ORIGINALS or original_count x recovery_count
 * > RS_LOCATE_MAX_COEFFICIENTS -> RS_ERR_INVALID_ARGUMENT.  Then every stripe's mask
 * is counted on the host, in stripe order.  A stripe that selects fewer than `need`
 * rows cannot be healed, and
 *   stripe_status == NULL: the call is all or nothing.  RS_ERR_INVALID_ARGUMENT with
 *     the first such stripe's number in err->index; nothing is launched, nothing
 *     is written, the context is not touched.
 *   stripe_status != NULL (HOST, `stripes` bytes): every stripe gets one rs_status,
 *     RS_OK or RS_ERR_INVALID_ARGUMENT.  A stripe that cannot be healed is skipped:
 *     none of its memory is read or written, its flags are all 0, d_located[b] =
 *     RS_LOCATE_SKIPPED and d_action[b] = 0.  The others are healed and the call
 *     returns RS_OK.
 * The matrices must not overlap one another or the three outputs.
 *   The table is the plain locate's and is shared every way: a stream warm from
 * rs_locate_device*, rs_heal_device* or this call builds none for any of the others.
 *   Launches, per 65535 stripes where the batch encode is one launch, else per
 * stripe: those of rs_locate_device_batch_masks (k_locate_find_masks also stores
 * the stripe's count of differing rows into per-stream scratch), then one
 * k_heal_masks directly after the group's k_locate_confirm_masks, while the group's
 * encode is still in scratch.  k_heal_masks has the confirm's grid; block (0, 0, b)
 * stores d_action[b], and the workgroups of a stripe with nothing to heal leave at
 * once.  A group in which no stripe can be healed has no confirm and no
 * k_heal_masks: where the batch has such a group, d_action is zeroed by a memset at
 * the start of the call, beside the flags' memset, and that zero is those stripes'
 * action (no heal launch; a batch without such a group has no memset of d_action,
 * since every k_heal_masks stores all the action bytes of its group).
 *   Measured (tools/heal_masks_time.py, profiles/heal_masks/heal_masks_time.txt;
 * 1024:1024, a random 10 % of every stripe's rows unselected, both mode bits,
 * max_rows 16, us per call, median of 5 rounds of 50 back-to-back calls, the legs
 * interleaved in one session; locate = rs_locate_device_batch_masks on the same
 * batch, spread = max - min of its five rounds; "parent" = that leg on the parent
 * commit's build in the same session, the yardstick; original / row = one corrupt
 * original / one corrupt selected row in EVERY stripe, net of the 5.0-5.7 us
 * launch that puts the damage back, and in brackets what the leg adds over the
 * clean locate beside what rs_heal_device_batch's leg adds over
 * rs_locate_device_batch; singles = one rs_heal_device per stripe):
 *     shape               parent spread  locate spread  heal clean  heal original         heal row            singles
 *     1 KiB, 64 stripes   259.24   1.15  259.83   4.53  262.27      288.88 (+29.1 | +28.8)  263.28 (+3.5 | +4.8)  1537.2
 *     64 KiB, one stripe  133.85   2.96  134.04   1.29  138.08      174.26 (+40.2 | +40.5)  141.09 (+7.1 | +4.4)   128.3
 * The expectation was: a clean batch costs the locate plus one small launch, i.e.
 * lies within the locate leg's spread plus one launch floor -- an empty-work k_heal
 * between two of the library's events, 6.2 us at both shapes in this session
 * (k_heal_masks 6.1 us at 64 stripes; 10.0 us in the one profiled clean call at
 * 64 KiB, 6.2 us in the next).  Met: +3.0 and +4.2 us over the parent's locate
 * (+2.4 and +4.0 over this build's).  The locate leg itself is +0.6 and +0.2 us
 * from the parent's, inside its own spread: the one optional store costs nothing
 * that shows.  A corrupt original adds what the shared-mask heal's adds, within
 * 0.3 us.  A corrupt row adds 1.4 us LESS than the shared-mask heal's at 64
 * stripes and 2.7 us MORE at 64 KiB, where the legs spread 0.4-1.3 us: that one is
 * outside the expectation, and the cause was not isolated (the clean call already
 * stands 2.1 us further above its locate than rs_heal_device_batch does above
 * its own; k_heal_masks' copy, 9.3 us, is k_heal's).  Against the 64-call loop of
 * rs_heal_device the call is 5.9 times cheaper; against rs_heal_device_batch with
 * every row selected it is 1.12 / 1.07 times dearer, which is the masks locate's
 * own distance from the plain locate (the staging copy of the row lists).
 * DESIGN.md §4.4l has the rest.
 *   Not covered: per-stripe masks for the robust and the degraded heal; a fused
 * form on k_mono_verify_masks; the host pipeline, the object API and the sharded
 * classes. */
rs_status rs_heal_device_batch_masks(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                     uint64_t recovery_count, uint64_t shard_bytes, uint64_t stripes,
                                     void *d_original, uint64_t original_stride, uint64_t original_stripe_stride,
                                     void *d_recovery, uint64_t recovery_stride, uint64_t recovery_stripe_stride,
                                     const uint8_t *recovery_check, uint32_t mode, uint32_t max_rows,
                                     int32_t *d_located, uint8_t *d_mismatch, uint8_t *d_action,
                                     uint8_t *stripe_status, void *stream, rs_error *err);

/* ---- robust heal: heal the original and its outlier rows, in place ----
 * rs_heal_device is built on the plain locate, so one rotten original plus a
 * flipped bit in some recovery row comes back RS_LOCATE_UNKNOWN with action 0, and
 * the caller is back to the three-call scrub: rs_locate_device_robust_batch, a
 * synchronize and a host read of three arrays, rs_repair_device_batch_masks.  Yet
 * after the robust locate everything a heal needs is on the device: d_located[b] =
 * i, the set B in d_outlier, the encode of the stored originals (want) in
 * per-stream scratch and the table log G.  The error is e = D_r / G[r][i] per
 * column for any selected row r outside B (each gives the same e, by the robust
 * locate's contract); the clean original is original_i ^ e; and the clean value of
 * a row j of B is want_j ^ G[j][i] * e, by the encode's linearity (the identity
 * rs_update_device rests on): encode(originals with e taken off original i)_j =
 * encode(stored originals)_j ^ G[j][i] * e.  This call is the robust locate
 * followed by one more launch per group of stripes that writes those: no decode,
 * no second encode, no host round trip.
 *   Arguments: those of rs_heal_device[_batch], in the same order, with
 * max_outliers before mode and d_outlier between d_mismatch and d_action.
 * Strides (0 = dense), alignment rules, the byte-wise path, the block and tail
 * layout and the HOST mask recovery_check (NULL = every row; ONE mask for every
 * stripe) are unchanged; rows marked 0 are never read and never written.
 * Asynchronous on `stream`; scratch per (context, stream).  With c = the number of
 * selected rows and t = max_outliers: 2 (1 + t) <= c, t <= RS_LOCATE_MAX_OUTLIERS.
 *   Result.  d_located, d_mismatch and d_outlier hold exactly what
 * rs_locate_device_robust_batch writes for the same arguments: they describe the
 * stripe AS FOUND.  Every byte of d_action is defined; it is a bit set, and unlike
 * rs_heal_device's it can be RS_HEAL_ORIGINAL | RS_HEAL_RECOVERY:
 *   d_located[b] = i >= 0, outlier set B
 *     RS_HEAL_ORIGINAL in mode: original i of stripe b has become original_i ^ e,
 *                     e = D_r / G[r][i] per column, r the first selected row
 *                     outside B.  Only its shard_bytes bytes are written, not the
 *                     row padding.  The action has the bit.
 *     RS_HEAL_RECOVERY in mode, B not empty: every row j of B of d_recovery has
 *                     become want_j ^ G[j][i] * e (a zero coefficient contributes
 *                     nothing), shard_bytes bytes per row.  The action has the
 *                     bit; with B empty it has not.  max_rows does not apply:
 *                     |B| <= max_outliers already.
 *     With both bits every selected row agrees afterwards; and if the true damage
 *     is s corrupt shards with s + 1 + t <= c (the robust locate's fact 2), both
 *     matrices are byte-identical to the clean stripe.  With one bit only the
 *     other half is left as found, and the next scan reports it: after
 *     RS_HEAL_ORIGINAL alone, RS_LOCATE_ROWS with exactly the rows of B flagged
 *     (which RS_HEAL_RECOVERY then rewrites, max_rows permitting); after
 *     RS_HEAL_RECOVERY alone, original i again, with no outliers -- by the plain
 *     locate as well.
 *   d_located[b] = RS_LOCATE_ROWS
 *                     exactly as rs_heal_device: RS_HEAL_RECOVERY in mode and at
 *                     most max_rows selected rows differ: each differing selected
 *                     row has become the encode of the stored originals, and the
 *                     action is RS_HEAL_RECOVERY.
 *   anything else     action 0, the stripe untouched.
 * Nothing else is written anywhere.  A second call on a stripe healed with both
 * bits reports RS_LOCATE_CLEAN, action 0, an all-zero d_outlier, and writes
 * nothing else.  With max_outliers == 0 the four outputs and both matrices equal
 * rs_heal_device_batch's for the same arguments, and d_outlier is all zero.
 *   CAVEATS.  The heal's "NOT proven", carried over: a ROWS stripe does not prove
 * the originals intact, and RS_HEAL_RECOVERY can make recovery rows consistent
 * with CORRUPT originals; keep max_rows well below half of the selected rows.  And
 * the robust locate's trust bound: beyond s + 1 + t <= c the located answer is a
 * codeword within 1 + t of the stored word, not necessarily the true one, and this
 * call writes it.  Keep t small against c.
 *   Errors, all before any device work, in this order: null context, d_original,
 * d_recovery, d_located, d_mismatch, d_outlier or d_action ->
 * RS_ERR_INVALID_ARGUMENT; rs_validate; the two row strides; mode == 0 or a bit
 * outside the two; fewer than 2 selected rows, or fewer than 3 with
 * RS_HEAL_ORIGINAL; max_outliers > RS_LOCATE_MAX_OUTLIERS or 2 (1 + max_outliers)
 * > c; the locate's shape bound -- each RS_ERR_INVALID_ARGUMENT.  At max_outliers
 * = 0 this is rs_heal_device_batch's order.  stripes == 0: RS_OK, nothing launched
 * or written, the context not touched.  The matrices must not overlap one another
 * or the four outputs.
 *   Launches: the robust locate's, its coefficient table shared with the locate,
 * the heal and the robust locate both ways; and one k_heal_robust per group of
 * stripes directly after that group's k_locate_decide, while the group's encode is
 * still in scratch (off the column kernel a group is one stripe and the scratch is
 * reused).  k_heal_robust has the confirm's grid; workgroups of a stripe with
 * nothing to do, and row groups with no row to write, leave at once.  On a located
 * stripe a workgroup finds r by a scan of at most t + 1 outlier bytes, forms e
 * once, row group 0 writes the original and every row group its rows of B; a ROWS
 * stripe's count of differing rows is summed from its flags by the workgroup.  No
 * ordering hazard by construction: e comes from row r and from scratch, neither
 * ever written; each pack of original i is read-modify-written by one lane; each
 * outlier row is written by the one workgroup that owns it, which reads only
 * scratch.
 *   Measured (tools/heal_robust_time.py,
 * profiles/heal_robust/heal_robust_time.txt; 1024:1024, every row, both mode bits,
 * max_rows 16, us per call, the legs interleaved in one session; locate =
 * rs_locate_device_robust_batch on the same inputs, whose kernels are the parent
 * commit's -- its legs on the parent's build in the same session read 33.83 /
 * 246.08 / 129.02 clean at t = 1 and 34.79 / 246.91 / 129.20 at t = 7
 * (heal_robust_time_parent.txt); spread = max - min of its five rounds; outlier =
 * one corrupt original plus a flipped bit in recovery row 0 of EVERY stripe, row =
 * one corrupt recovery row in every stripe; scrub = the three calls with their
 * synchronize, host read and masks for the outlier damage; the damaged heal and
 * scrub legs net of the 4.3-6.4 us launch that puts the damage back):
 *     shape, t              locate clean (spread) / outlier / row   heal clean / outlier / row    scrub outlier
 *     1 KiB, one stripe, 1   27.33 (2.90) /  33.14 /  31.99          35.10 /  35.56 /  36.32       140.84
 *     1 KiB, one stripe, 7   26.55 (0.28) /  39.18 /  32.81          35.26 /  41.81 /  36.45       146.52
 *     1 KiB, 64 stripes, 1  247.23 (1.32) / 289.74 / 247.60         249.07 / 302.53 / 253.65      1074.69
 *     1 KiB, 64 stripes, 7  247.46 (0.68) / 324.88 / 247.95         249.06 / 338.11 / 254.00      1108.66
 *     64 KiB, one stripe, 1 132.55 (1.21) / 189.86 / 130.44         134.02 / 196.38 / 136.07       494.20
 *     64 KiB, one stripe, 7 132.94 (0.85) / 216.84 / 131.51         134.78 / 223.41 / 136.98       522.24
 * A clean heal costs the robust locate plus one small launch, k_heal_robust at the
 * 6.1-6.2 us floor by the events: +1.8 / +1.6 us on 64 stripes and +1.5 / +1.8 us
 * at 64 KiB, inside the yardstick's spread plus one floor as expected.  The single
 * 1 KiB stripe reads +7.8 us at t = 1 (spread 2.9: inside) and +8.7 us at t = 7
 * (spread 0.3: 2 us OUTSIDE the expectation); that shape is launch-bound and
 * moved by as much between two processes of the same kernels (the parent's
 * build read 33.8 / 34.8 us for the 27.3 / 26.6 us leg).  A damaged heal costs the
 * robust locate's damaged case plus that launch: +2.4 / +12.8 / +6.5 us at t = 1
 * and +2.6 / +13.2 / +6.6 us at t = 7 for the outlier case (k_heal_robust 8.8 /
 * 16.0 / 10.2 us by the events: one original and one row read and written per
 * stripe), +3.7-4.3 / +6.1 / +5.5 us for a row.  It beats the three-call scrub by
 * 105 / 772 / 298 us (4.0 / 3.6 / 2.5 times at t = 1, 3.5 / 3.3 / 2.3 at t = 7),
 * more than the scrub's decode (k_mono_repair_masks 20 / 614 us, the 64 KiB
 * decode's launches 212 us by the events), the rest being the synchronize, the
 * three reads on the host and the masks.  DESIGN.md "Robust heal" has the rest.
 *   Not covered: two or more corrupt originals; a mask per stripe; stripes with
 * missing originals (rs_locate_device_degraded above locates in those); the host
 * pipeline, the object API and the sharded classes. */
rs_status rs_heal_device_robust(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                uint64_t shard_bytes, void *d_original, uint64_t original_stride, void *d_recovery,
                                uint64_t recovery_stride, const uint8_t *recovery_check, uint32_t max_outliers,
                                uint32_t mode, uint32_t max_rows, int32_t *d_located, uint8_t *d_mismatch,
                                uint8_t *d_outlier, uint8_t *d_action, void *stream, rs_error *err);
rs_status rs_heal_device_robust_batch(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                      uint64_t shard_bytes, uint64_t stripes, void *d_original,
                                      uint64_t original_stride, uint64_t original_stripe_stride, void *d_recovery,
                                      uint64_t recovery_stride, uint64_t recovery_stripe_stride,
                                      const uint8_t *recovery_check, uint32_t max_outliers, uint32_t mode,
                                      uint32_t max_rows, int32_t *d_located, uint8_t *d_mismatch, uint8_t *d_outlier,
                                      uint8_t *d_action, void *stream, rs_error *err);

/* ---- degraded heal: fix what the degraded locate found, in place ----
 * rs_locate_device_degraded names the corrupt information shard of a stripe that
 * has originals missing, and leaves the caller to act on it: a synchronize, a host
 * read of d_located, masks per stripe and rs_repair_device_batch_masks, a second
 * full decode of every damaged stripe -- on the stripes where a disk is already
 * out and every restored original carries the error.  Yet at the end of the
 * degraded locate everything a heal needs is on the device: the located position
 * q, e = D_j0 / T[j0][q] per column (j0 = K[0]), which the confirm has just formed,
 * the completed stripe's recovery rows in per-stream scratch, and the restored
 * originals in d_restored.  The missing ingredient is U[p][q], the element that the
 * decode from R puts into restored original p when information position q holds
 * the element 1 and every other one holds zero: the decode is linear per column,
 * so with shard q wrong by e
 *     clean shard q            = stored shard q ^ e
 *     clean missing original p = F_b[p] ^ U[p][q] * e.
 * No U[p][q] is zero (the codeword with 1 at q and 0 at the other original_count - 1
 * information positions would have original_count zeros; an MDS code allows one
 * fewer).  This call is the degraded locate followed by one more launch per group of
 * stripes that writes those: asynchronous on `stream`, no host synchronization, no
 * second decode.  Notation is rs_locate_device_degraded's.
 *   Arguments.  Argument order, the two HOST masks (ONE of each for every stripe of
 * a batch), strides (0 = dense), alignment rules, the byte-wise path and the block
 * and tail layout are those of rs_locate_device_degraded[_batch]; mode, max_rows and
 * d_action those of rs_heal_device.  d_original and d_recovery are written in place.
 * d_restored is REQUIRED; it may alias d_original with equal strides.
 *   Result.  d_located and d_mismatch hold exactly what
 * rs_locate_device_degraded_batch writes for the same arguments: they describe the
 * stripe AS FOUND.  Every byte of d_action is defined:
 *   RS_HEAL_ORIGINAL  d_located[b] = i < original_count (a present original) and mode
 *                     has the bit: original i has become original_i ^ e, and every
 *                     missing original's row p of d_restored F_b[p] ^ U[p][i] * e.
 *                     Only shard_bytes bytes per row are written.
 *   RS_HEAL_RECOVERY  d_located[b] = original_count + j (a reference row) and mode has
 *                     the bit: recovery row j has become recovery_j ^ e, and the
 *                     restored rows are corrected the same way with that row's
 *                     position.  Or d_located[b] = RS_LOCATE_ROWS, mode has the bit
 *                     and at most max_rows rows of K differ: each differing row of K
 *                     has become the encode of F_b; the restored rows stay F_b's.
 *   0                 anything else (CLEAN, UNKNOWN, ROWS above the threshold, an
 *                     outcome whose mode bit is off): the three matrices end up
 *                     exactly as rs_locate_device_degraded_batch leaves them -- the
 *                     missing rows of d_restored are F_b's, nothing else is written.
 * The mode bits say which matrix the call may write: RS_HEAL_ORIGINAL d_original,
 * RS_HEAL_RECOVERY d_recovery (d_restored is written by every call).
 *   After a located stripe is healed every selected row, R and K alike, agrees
 * with the encode of the now complete originals; if that shard was the only
 * damage, d_original with d_restored's rows, and d_recovery, are byte-identical to
 * the clean stripe; a second call on the result reports RS_LOCATE_CLEAN with action
 * 0 and rewrites the missing rows with the same bytes.
 *   CAVEAT (the heal's, carried over): a ROWS stripe does not prove the information
 * shards intact; RS_HEAL_RECOVERY can make check rows consistent with CORRUPT ones.
 * Keep max_rows well below half of |K|.
 *   m == 0: the call delegates to rs_heal_device_batch and leaves d_restored
 * untouched.
 *   Errors, all before any device work, in this order: null context, d_original,
 * original_present, d_recovery, d_restored, d_located, d_mismatch or d_action ->
 * RS_ERR_INVALID_ARGUMENT; rs_validate; the three row strides; mode == 0 or a bit
 * outside the two -> RS_ERR_INVALID_ARGUMENT; c < m -> RS_ERR_NOT_ENOUGH_SHARDS with
 * the decode's counts; c < m + 3 -> RS_ERR_INVALID_ARGUMENT (the call writes on the
 * evidence of a location, so it takes three check rows: with two, two corrupt
 * information shards can be attributed to a third, see the degraded locate); the
 * locate's shape bound.  stripes == 0: RS_OK, nothing launched or written, the
 * context not touched.  The matrices must not overlap one another or the three
 * outputs, d_restored on d_original excepted.
 *   Launches: the degraded locate's, group of stripes by group of stripes;
 * k_locate_find also stores each stripe's count of differing rows; and one
 * k_heal_degraded per group directly after that group's k_locate_confirm and before
 * its k_locate_rename, while d_located[b] is still the information position and the
 * group's `want` is still in scratch.  Its grid is the confirm's pack tiles x row
 * groups over max(m, |K|) rows x stripes; a located stripe's restored rows are dealt
 * round the row groups; workgroups of a stripe with nothing to do, and row groups
 * with no row, leave at once.
 *   The table log U[r][q], m x original_count uint16_t (row r: the r-th missing
 * original), is kept beside log T under the same key.  It comes from the first output
 * of the unit stripe's repair, which the degraded locate's table build discards: one
 * k_coef_log_rows per slab right after that slab's repair, and only when a heal asks
 * for it -- rs_locate_device_degraded launches exactly what it did.  A degraded locate
 * after a heal on the stream finds T.  A heal after a degraded locate builds BOTH
 * tables again: the slab's repair, which is the cost, yields both at once.
 *   Measured (tools/heal_degraded_time.py, profiles/heal_degraded/heal_degraded_time.txt;
 * 1024:1024, every row, both mode bits, max_rows 16, d_restored = d_original, us per
 * call, median of five rounds of 50 back-to-back calls, the legs interleaved in one
 * session; locate = rs_locate_device_degraded_batch on the clean batch, spread = max -
 * min of its five rounds, in brackets the same leg on the parent commit's build in
 * the same session; corrupt = one corrupt present original in EVERY stripe; scrub =
 * what a caller had before: the degraded locate, a synchronize, a host read of
 * d_located, the masks and rs_repair_device_batch_masks with the named shard absent;
 * the corrupt heal and scrub legs net of the 4.6-5.6 us launch that puts the damage
 * back before each call):
 *     shape, m                locate (parent) spread  heal clean  locate corrupt  heal corrupt  scrub corrupt
 *     1 KiB, one stripe, 1     26.40  (29.17)   2.25     33.22        34.88           36.30        104.36
 *     1 KiB, one stripe, 16    28.17  (29.51)   5.69     33.03        35.00           36.33        110.16
 *     1 KiB, 64 stripes, 1    536.28 (535.56)   1.27    539.41       565.45          572.13       1309.73
 *     1 KiB, 64 stripes, 16   559.68 (559.08)   1.36    562.43       589.59          595.57       1335.48
 *     64 KiB, one stripe, 1   249.84 (249.30)   3.16    252.35       291.75          296.94        506.52
 *     64 KiB, one stripe, 16  292.48 (292.32)   0.61    294.94       336.98          343.61        595.23
 * The expectation was "the degraded locate on the same input plus one launch": on a
 * clean batch within the locate's spread plus one launch floor (6.0-6.2 us, the
 * shortest launch of the call by the library's events), on a damaged stripe a
 * read-modify-write of m + 1 rows more.  On 64 stripes and at 64 KiB every clean case
 * lands well within it: +3.1 / +2.7 and +2.5 / +2.5 us, k_heal_degraded at 6.0-6.5 us
 * between two of the library's events.  The single 1 KiB stripe is bound by the host's
 * launch rate (six launches in 26-28 us), and there the seventh launch costs +6.8 /
 * +4.9 us: within the bound as the tool computes it, but only because that leg's rounds
 * spread 2.3-5.7 us.  A second session of the same build, right after the whole test
 * suite (heal_degraded_time_after_suite.txt), read +8.2 / +8.7 us there, the second 1.0
 * us OUTSIDE its bound of 7.7 us; its other four cases read +0.8 to +3.3 us.  So at one
 * small stripe a clean heal costs the locate plus 5-9 us, about one launch slot of the
 * host's, not the 2-3 us of the larger cases -- as rs_heal_device_robust measured on
 * the same shape.  The locate legs of this build and of the parent's agree within
 * 0.2-0.7 us (1.3-2.8 us on the single stripe, inside that leg's spread): the locate
 * launches what it did.  A healed original costs +1.4 / +1.3 us over the locate's own
 * corrupt case on the single stripe, +6.7 / +6.0 us on 64 stripes and +5.2 / +6.6 us at
 * 64 KiB (k_heal_degraded 6.5 / 9.6-8.0 / 7.6 us by the events): the restored rows of a
 * located stripe are dealt round the grid's row groups, so that m = 16 under 1008
 * check rows spreads over 16 workgroups per pack tile and costs what m = 1 does.
 * (The corrupt heal's figures are a difference: each call is timed behind the launch
 * that puts the damage back, and that launch's median, 4.6-5.6 us timed alone with
 * rounds spreading 0.1-2.0 us, is taken off; on the single stripe it may also overlap
 * the call's own launches on the host.  So these deltas are good to about 2 us, and
 * the single stripe's +1.4 / +1.3 us says "at most a few us", no more; the kernel's
 * device time by the events is the direct figure.)
 * Both beat the scrub by more than its second decode (k_mono_repair_masks 19.5 / 606-610 us, the 64
 * KiB decode's launches 169 / 219 us by the events): by 68 / 74 us (2.9 / 3.0 times) on
 * the single stripe, 738 / 740 us (2.3 / 2.2 times) on 64 stripes and 210 / 252 us (1.7
 * times) at 64 KiB, the rest being the synchronize, the read and the masks.
 * DESIGN.md "Degraded heal" has the rest.
 *   Not covered: max_outliers for degraded stripes; a mask per stripe; filling
 * unselected recovery rows; the host pipeline, the object API and the sharded
 * classes. */
rs_status rs_heal_device_degraded(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                                  uint64_t shard_bytes, void *d_original, uint64_t original_stride,
                                  const uint8_t *original_present, void *d_recovery, uint64_t recovery_stride,
                                  const uint8_t *recovery_check, void *d_restored, uint64_t restored_stride,
                                  uint32_t mode, uint32_t max_rows, int32_t *d_located, uint8_t *d_mismatch,
                                  uint8_t *d_action, void *stream, rs_error *err);
rs_status rs_heal_device_degraded_batch(rs_context *ctx, rs_rate rate, uint64_t original_count,
                                        uint64_t recovery_count, uint64_t shard_bytes, uint64_t stripes,
                                        void *d_original, uint64_t original_stride, uint64_t original_stripe_stride,
                                        const uint8_t *original_present, void *d_recovery, uint64_t recovery_stride,
                                        uint64_t recovery_stripe_stride, const uint8_t *recovery_check,
                                        void *d_restored, uint64_t restored_stride, uint64_t restored_stripe_stride,
                                        uint32_t mode, uint32_t max_rows, int32_t *d_located, uint8_t *d_mismatch,
                                        uint8_t *d_action, void *stream, rs_error *err);

/* ---- host-memory pipeline (shards arrive from a socket or file) ----
 * h_original (original_count x shard_bytes) and h_recovery (recovery_count x
 * shard_bytes) are row-major HOST matrices; pinned memory (rs_host_alloc,
 * hipHostMalloc) gives full PCIe rate, pageable memory works but is staged by
 * the runtime.  The byte axis is cut into `slices` column slices of whole
 * 64-byte blocks (0 = 1); slice k is copied in, coded and copied out on its
 * own stream, overlapping neighbouring slices.  Blocking: returns when the
 * outputs are in host memory.  shard_bytes: any even size (the tail block
 * travels with the last slice).
 * Decode copies in only received rows and writes only the missing originals
 * of h_restored (original_count x shard_bytes). */
void *rs_host_alloc(uint64_t bytes);
void rs_host_free(void *p);
rs_status rs_encode_host(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                         uint64_t shard_bytes, const void *h_original, void *h_recovery, uint32_t slices,
                         rs_error *err);
rs_status rs_decode_host(rs_context *ctx, rs_rate rate, uint64_t original_count, uint64_t recovery_count,
                         uint64_t shard_bytes, const void *h_original, const uint8_t *original_present,
                         const void *h_recovery, const uint8_t *recovery_present, void *h_restored,
                         uint32_t slices, rs_error *err);

/* ---- Engine trait over a device shard matrix (src/engine.rs:234-291) ----
 * d_rows: shard_count rows of shard_len_64 64-byte blocks (ShardsRefMut,
 * src/engine/shards.rs:100-189).  Infallible in the reference (debug_assert on
 * bad args); here bad args return RS_ERR_INVALID_ARGUMENT.  Semantics are
 * engine_naive.rs:43-105 for every row, including rows at and past
 * truncated_size (only the butterfly groups that start below it are
 * transformed). */
rs_status rs_engine_fft(rs_context *ctx, void *d_rows, uint64_t shard_count, uint64_t shard_len_64, uint64_t pos,
                        uint64_t size, uint64_t truncated_size, uint64_t skew_delta, void *stream);
rs_status rs_engine_ifft(rs_context *ctx, void *d_rows, uint64_t shard_count, uint64_t shard_len_64, uint64_t pos,
                         uint64_t size, uint64_t truncated_size, uint64_t skew_delta, void *stream);
rs_status rs_engine_mul(rs_context *ctx, void *d_rows, uint64_t block_count, uint16_t log_m, void *stream);
/* host array of 65536 elements, in place (src/engine/utils.rs:20-31) */
void rs_engine_eval_poly(uint16_t *erasures, uint64_t truncated_size);
/* formal derivative over all shard_count rows (src/engine/utils.rs:99-104) */
rs_status rs_engine_formal_derivative(rs_context *ctx, void *d_rows, uint64_t shard_count, uint64_t shard_len_64,
                                      void *stream);

/* ---- Engine trait over a HOST shard array: the reference's own calling convention ----
 * `rows` is the host storage of a ShardsRefMut (shard_count x shard_len_64 64-byte
 * blocks, src/engine/shards.rs:100-189); Engine::fft / ifft (src/engine.rs:119-151)
 * transform rows [pos, pos + size) and Engine::mul (src/engine.rs:154) scales
 * block_count blocks.  Blocking: the rows are copied to the device, transformed
 * with the same kernels as rs_engine_fft / rs_engine_ifft / rs_engine_mul, and
 * copied back.  This is what a Rust `impl Engine` binds; it pays a
 * PCIe round trip per call, the device-resident calls above do not. */
rs_status rs_engine_fft_host(rs_context *ctx, uint8_t *rows, uint64_t shard_count, uint64_t shard_len_64,
                             uint64_t pos, uint64_t size, uint64_t truncated_size, uint64_t skew_delta);
rs_status rs_engine_ifft_host(rs_context *ctx, uint8_t *rows, uint64_t shard_count, uint64_t shard_len_64,
                              uint64_t pos, uint64_t size, uint64_t truncated_size, uint64_t skew_delta);
rs_status rs_engine_mul_host(rs_context *ctx, uint8_t *blocks, uint64_t block_count, uint16_t log_m);

/* Device scratch of one stream (see "Thread-safety"): synchronizes `stream`
 * and frees the context's scratch for it.  The stream must still be valid. */
#define RS_MAX_STREAM_WORKSPACES 16
rs_status rs_release_stream_scratch(rs_context *ctx, void *stream);

/* ---- kernel timing (bench instrumentation, not a reference item) ----
 * While enabled, every kernel the context launches is bracketed by HIP events
 * on the stream it is launched on.  rs_profile_collect synchronizes those
 * events and returns, in launch order, each launch's duration (ms), its
 * kernel name and the algorithmic HBM bytes of that launch (rows it must read
 * from memory + rows it writes, times the row size); then clears the record.
 * Returns the number of records written (<= max). */
rs_status rs_profile_enable(rs_context *ctx, int enable);
int rs_profile_collect(rs_context *ctx, float *ms, uint64_t *bytes, const char **names, int max);

/* ---- device check ----
 * rs_check_device synchronizes the context's device and returns
 * RS_ERR_DEVICE (message in rs_last_device_error) if an earlier asynchronous
 * launch failed, else RS_OK. */
rs_status rs_check_device(rs_context *ctx);

/* ---- column kernel control (engine tuning, not a reference item) ----
 * Transforms of 2^7 .. 2^12 rows over at most RS_MI355X_MONO_MAX_PACKS (256)
 * packs of 4 elements run as one launch in which a workgroup owns every row
 * of one pack (DESIGN.md "Column kernel").  rs_mono_enable(ctx, 0) selects
 * the pass kernels instead (also: RS_MI355X_NO_MONO=1 at context
 * creation); 1 (default) uses it where it is fastest (single-chunk transforms
 * of 2^7 .. 2^10 rows, twiddles staged in LDS); 2 also for multi-chunk and
 * 2^11 / 2^12-row transforms (also: RS_MI355X_MONO_ALL=1).  Adding 4 turns off
 * the split decode plan of 2^9 .. 2^11-row decodes whose restored rows lie in
 * one half of the work rows (also: RS_MI355X_NO_SPLIT=1).  Single-chunk
 * encodes and decodes of at most half the device's CU count of 4-element packs
 * use packs of 2 elements (twice the workgroups; RS_MI355X_E2_MAX_PACKS sets
 * the limit): adding 8 keeps 4-element packs, adding 16 uses 2-element packs
 * for every single-chunk launch.  Single-chunk 2-element encodes of 2^8 and 2^9
 * rows run on the one-row-per-lane kernel (rs_lane.hip; RS_MI355X_LANE=0 at
 * context creation: never); adding 32 also runs 2^10-row ones there, adding 64
 * none.  Adding 128 runs single-chunk transforms of 2^12 rows as two launches
 * of the 2^11-row kernel split by halves of the rows (off by default: slower
 * than the pass kernels; RS_MI355X_HALF=1 at context creation: on), adding 256
 * turns that off again.  Multi-chunk encodes of 2^2 .. 2^7-row transforms
 * (HighRate N > pow2(M), LowRate M > pow2(N)) run as one launch whose waves
 * take the chunks in parallel (rs_chunks.hip; RS_MI355X_CHUNKS=0 at context
 * creation: never) where that measured faster: all of them but LowRate
 * encodes of more than 8 output chunks in 2-element packs.  Adding 512 sends
 * every multi-chunk encode of those sizes there, adding 1024 none.  Adding
 * 2048 runs single-chunk 2-element encodes of 2^10 rows as the 4-element
 * kernel of 2^9 pair rows (the quad encode; off by default: bit-exact but
 * slower; RS_MI355X_QUAD=1 at context creation: on), adding 4096 turns it off.
 * Single-chunk encodes of N = M = 2^7 .. 2^11 shards of whole 64-byte blocks,
 * 4-byte aligned, every recovery row asked for, run the column kernel's dense
 * entry, which takes the row maps' geometry as decided by the host instead of
 * testing it per lane (on by default; RS_MI355X_DENSE=0 at context creation:
 * never): adding 8192 turns it on, adding 16384 off (the general entry).
 * Where the dense entry runs an encode of N = M = 2^10 shards in 2-element
 * column packs (at most half the device's CUs in 8-byte packs), one stripe, its
 * split form can run instead: a pair of rows' two byte planes on neighbouring
 * lanes, half multiplies (RS_ENC_SPLIT_DEFAULT; RS_MI355X_ENC_SPLIT=0/1 at
 * context creation): adding 32768 turns it on, adding 65536 off.  With the dense
 * entry off the split form is off too.
 * Neither bit of a pair: the context's defaults (its environment included).
 * A/B and tests; results are identical in every mode. */
rs_status rs_mono_enable(rs_context *ctx, int enable);
/* Launches of the dense entry by this process so far (tests, A/B: the profile
 * records name the general and the dense entry alike, k_mono<...>).  A launch
 * of the split form counts here too. */
uint64_t rs_mono_dense_launches(void);
/* The split form of the dense entry: the default of a new context (measured,
 * DESIGN.md 9), and its launches by this process so far. */
#define RS_ENC_SPLIT_DEFAULT 1
uint64_t rs_mono_split_launches(void);

/* ---- GF(2^16) tables (src/engine/tables.rs), host copies ---- */
const uint16_t *rs_table_exp(void);       /* 65536 */
const uint16_t *rs_table_log(void);       /* 65536 */
const uint16_t *rs_table_skew(void);      /* 65535 */
const uint16_t *rs_table_log_walsh(void); /* 65536 */
/* this engine's byte-permute multiply tables, 20 words per entry, 65536
 * entries (format: reed-solomon-simd_amd/csrc/gf_tables.cpp fill_perm) */
const uint32_t *rs_table_perm_by_log(void);
const uint32_t *rs_table_perm_by_skew(void);

#ifdef __cplusplus
}
#endif
#endif
