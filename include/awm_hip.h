/* awm_hip.h -- C ABI of the MI355X (gfx950) spectral watermark path.
 *
 * The reference (swesterfeld/audiowmark 0.6.5) has no FFI layer; the seams this library
 * replaces are C++ member functions.  Each entry point below names the reference
 * interface it stands in for (file:line relative to the reference's src/).
 *
 * Conventions
 *   - plain C, pointers + sizes only.  Pointers suffixed _d are DEVICE pointers (HBM),
 *     everything else is host memory.
 *   - device buffers need only the alignment of their element type (4 bytes for float32
 *     PCM and tables, 1 byte for raw PCM bytes and flags): results are bit-identical at every
 *     placement and nothing outside [pointer, pointer + size) is read or written
 *     (tests/test_gpu_placement.py is that promise).
 *   - return 0 on success, negative on error; awm_last_error() gives the message
 *     (thread-local).  There is NO CPU fallback: without a usable gfx950 device every
 *     compute entry point fails with AWM_ERR_NO_DEVICE.
 *   - PCM is interleaved float32, `n_frames` = samples per channel (reference WavData,
 *     wavdata.hh:27-74); all watermark arithmetic is at 44100 Hz (wmcommon.hh:68).
 *   - work is enqueued on the context's HIP stream; entry points that return host data
 *     synchronise that stream before returning, the *_async ones do not.
 */
#ifndef AWM_HIP_H
#define AWM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AWM_ERR_GENERIC    (-1)
#define AWM_ERR_NO_DEVICE  (-2)
#define AWM_ERR_ARG        (-3)
#define AWM_ERR_HIP        (-4)
#define AWM_ERR_IO         (-5)    /* a file could not be opened / read / written (file level entry points) */

#define AWM_FRAME_SIZE      1024
#define AWM_N_BANDS         81      /* bins 20..100, wmcommon.hh:39-40 */
#define AWM_BLOCK_FRAMES    2226    /* 510 sync + 1716 data frames at the default payload */
#define AWM_SOFT_BITS       858     /* conv_code_size(a,128), convcode.cc:65-75 */

typedef struct awm_ctx awm_ctx;

const char *awm_last_error (void);
const char *awm_version (void);

/* ---- context: one per GPU / per rank ------------------------------------------------ */
int   awm_ctx_create (int device, awm_ctx **ctx_out);
/* the same on a stream of the caller (NULL: the device's default stream); the context then creates no stream of its own
 * (every HIP stream costs ~190 MB of resident host memory on this runtime: the command line uses this) */
int   awm_ctx_create_on_stream (int device, void *hip_stream, awm_ctx **ctx_out);
void  awm_ctx_destroy (awm_ctx *ctx);
/* A context keeps its workspaces between calls (a call's set-up is then ~1.5 ms instead of 20 - 25): the lanes' scratch buffers, the
 * file level staging rings (4 + 4 page-locked tiles of up to 32 MiB and their device twins) and the float32 PCM of the longest stream the
 * file level `get` has decoded (1.3 GB per hour).  awm_ctx_trim gives all of that back (also for the context's helpers); key tables and
 * streams stay.  For long-lived services after an unusually long file. */
int   awm_ctx_trim (awm_ctx *ctx);
/* ... and the other way round: create NOW the HIP streams a first call would create (4 - 10 ms each in this runtime): the chunk lanes of
 * `get` (twice as many with detect_speed != 0: the plain decode runs beside the speed search), with file_level != 0 the copy stream of the
 * file level calls.  For services that create their contexts at start-up. */
int   awm_ctx_warm_up (awm_ctx *ctx, int detect_speed, int file_level);
int   awm_ctx_device (const awm_ctx *ctx);
int   awm_ctx_synchronize (awm_ctx *ctx);
/* opaque hipStream_t of the context (for callers that bracket work with HIP events) */
void *awm_ctx_stream (awm_ctx *ctx);
/* run all work of this context on an externally owned hipStream_t (e.g. torch's current stream) */
int   awm_ctx_set_stream (awm_ctx *ctx, void *hip_stream);
/* `get` decodes the 30-minute chunks of a stream concurrently on up to 4 "lanes" (HIP streams with their own workspaces);
 * n_lanes = 1 runs them one after the other on the context's stream (per-kernel timing without overlap, smallest footprint) */
int   awm_ctx_set_chunk_lanes (awm_ctx *ctx, int n_lanes);

/* ---- per-kernel timing: HIP events recorded on the context's stream around every launch.
 * ids 0..awm_prof_count()-1, awm_prof_name(id) is the kernel name as rocprofv3 shows it (plus the
 * call site in brackets); algorithmic_bytes = SURVEY.md section 8(d) bytes summed over the launches. */
int         awm_prof_enable (awm_ctx *ctx, int on);
int         awm_prof_reset (awm_ctx *ctx);
int         awm_prof_count (void);
const char *awm_prof_name (int id);
int         awm_prof_read (awm_ctx *ctx, int id, double *ms, long *launches, double *algorithmic_bytes);

/* ---- key-derived tables (pure host, callable without a GPU) -------------------------- */
/* replaces: UpDownGen::get wmcommon.hh:107-122; BitPosGen wmcommon.cc:143-165;
 *           gen_mix_entries wmcommon.cc:179-202; init_frame_mod_vec wmadd.cc:148-162;
 *           SyncFinder::get_sync_bits syncfinder.cc:30-77; randomize_bit_order wmcommon.hh:165-185 */
int awm_tab_up_down (const uint8_t key[16], int stream, int frame, int up[30], int down[30]);
int awm_tab_bit_pos (const uint8_t key[16], int pos[AWM_BLOCK_FRAMES]);
int awm_tab_mix_entries (const uint8_t key[16], int *frame_up_down /* [51480*3] */);
int awm_tab_bit_order (const uint8_t key[16], size_t n, unsigned *order);
/* out[2][2226][81]: 0 KEEP / 1 UP / 2 DOWN for the A and the B block */
int awm_tab_frame_mod (const uint8_t key[16], const char *payload_hex, int8_t *out);
/* what of that table depends on the key alone, out[2][block frames][81] int16: 0 KEEP / 1 UP / 2 DOWN (the sync frames of the block
 * type) or 4 + 2 k + s, a data band governed by bit k of conv_encode (block type, payload) -- k BEFORE the bit order, which is folded in;
 * s = 0: UP when the bit is 1, DOWN otherwise; s = 1 the opposite.  The walk of wmadd.cc:86-162, write for write: expanded with a
 * payload's A and B code it is awm_tab_frame_mod of that payload byte for byte (mix and frames_per_bit as in force).  Returns the
 * number of entries; with out == NULL that number alone (nothing is written), so that a caller can size the buffer. */
int awm_tab_frame_mod_template (const uint8_t key[16], int16_t *out);
/* out rows: frame, up[30], down[30] (band-20, ascending); returns rows per bit (85 / 170) */
int awm_tab_sync_bits (const uint8_t key[16], int clip_mode, int *out /* [6*rows*61] */);
int awm_tab_window (size_t n, float *out);                    /* FFTAnalyzer::gen_normalized_window wmcommon.cc:68-89 */
int awm_tab_synth_window (float *out /* [3072] */);           /* WatermarkSynth::generate_window wmadd.cc:177-206 */
int awm_conv_encode (int block_type, const int *bits, size_t n, int *out); /* conv_encode convcode.cc:100-125 */
/* `audiowmark test-gen-noise` (audiowmark.cc:399-417): n_values floats = rng.random_double() * 2 - 1 of
 * Random (key, 0, Stream::data_up_down) -- the reference's own synthetic input (interleaved stereo white noise) */
int awm_test_gen_noise (const uint8_t key[16], size_t n_values, float *out);

/* ---- kernel level (device pointers) --------------------------------------------------- */

/* FFTAnalyzer::run_fft / fft_range (wmcommon.cc:91-141): `frame_count` windowed 1024-point
 * r2c transforms per channel, frame f starting at sample start_index + f*hop.
 * out_d: [frame_count][n_channels][513] complex64 (re,im).  Fails if the range exceeds n_frames. */
int awm_stft_d (awm_ctx *ctx, const float *pcm_d, size_t n_frames, int n_channels,
                size_t start_index, size_t hop, size_t frame_count, float *out_d);

/* add: WatermarkGen::run + WatermarkSynth::run + mix + Limiter (wmadd.cc:61-84,215-250,297-317,
 * 564-568; limiter.cc:90-124) for a contiguous span of the stream.
 *   frame_mod:        host table from awm_tab_frame_mod ([2][2226][81])
 *   first_frame:      index (in 1024-sample frames) of pcm_in_d[0] inside the whole stream; spans
 *                     are how awm shards `add` across GPUs.  The span must start on a frame boundary.
 *   halo_before_d / halo_after_d: the 1024*C samples preceding / following the span (NULL = stream
 *                     start / zeros after the end), needed for the 3-frame overlap-add (wmadd.cc:228-238)
 *   use_limiter:      0 = Params::test_no_limiter
 * awm_add_mix_d writes the un-limited mix to out_d and accumulates per-limiter-block maxima into
 * block_max_d[b] (b = global limiter block index - first_block, float32, pre-initialised by
 * awm_add_init_block_max_d); awm_add_limit_d applies the limiter ramp in place.  Between the two a
 * multi-GPU caller all-reduces (max) block_max_d.  awm_add_d = both, single GPU.
 * Every output frame is computed from three input frames: out_d must not overlap pcm_in_d.  awm_add_d refuses an output that overlaps
 * the input anywhere (AWM_ERR_ARG, nothing enqueued). */
int awm_add_init_block_max_d (awm_ctx *ctx, float *block_max_d, size_t n_blocks);
int awm_add_mix_d (awm_ctx *ctx, const float *pcm_in_d, float *out_d, size_t n_frames, int n_channels,
                   const int8_t *frame_mod, double water_delta, size_t first_frame,
                   const float *halo_before_d, const float *halo_after_d,
                   float *block_max_d /* may be NULL: no limiter */, size_t first_block, size_t n_blocks);
int awm_add_limit_d (awm_ctx *ctx, float *out_d, size_t n_frames, int n_channels, size_t first_sample,
                     const float *block_max_d, size_t first_block, size_t n_blocks);
/* The two halves on SIGNED 16-BIT PCM (whole streams from and to 16-bit PCM: awm_add_watermark_s16_d below).
 * awm_add_mix_s16_d is K2 instantiated for 16-bit input, span form included: pcm_in_d and the halos are int16 values (little-endian,
 * interleaved, any even address), converted where they leave global memory; out_d (float) and block_max_d are bit for bit what
 * awm_add_mix_d writes for the stream and the halos decoded by awm_pcm_decode_d (float (v) * (1 / 32768)).  The rules are awm_add_mix_d's:
 * the span starts on a frame boundary, a NULL block_max_d means no limiter, the maxima are pre-initialised with awm_add_init_block_max_d.
 * awm_add_limit_s16_d is the last pass: out_d (int16) is value for value what awm_pcm_encode_d (..., 16, 0, 0, direct16 = 1, out_d) writes
 * for what awm_add_limit_d leaves in a copy of mix_d -- ramp, v * 32768, saturated at 32767 and -32768, truncated, in one pass.  mix_d is
 * not modified, nothing outside [out_d, out_d + n C) is written; block_max_d NULL: no ramp.  Stereo on a 4-byte aligned out_d stores
 * groups of four frames (16 bytes), mono groups of eight values, everything else a value per thread.
 * AWM_ERR_ARG with nothing enqueued: a NULL pointer with n_frames > 0, n_channels < 1, an int16 pointer at an odd address. */
int awm_add_mix_s16_d (awm_ctx *ctx, const int16_t *pcm_in_d, float *out_d, size_t n_frames, int n_channels,
                       const int8_t *frame_mod, double water_delta, size_t first_frame,
                       const int16_t *halo_before_d, const int16_t *halo_after_d,
                       float *block_max_d /* may be NULL: no limiter */, size_t first_block, size_t n_blocks);
int awm_add_limit_s16_d (awm_ctx *ctx, const float *mix_d, int16_t *out_d, size_t n_frames, int n_channels, size_t first_sample,
                         const float *block_max_d /* NULL: no ramp */, size_t first_block, size_t n_blocks);
int awm_add_d (awm_ctx *ctx, const float *pcm_in_d, float *out_d, size_t n_frames, int n_channels,
               const int8_t *frame_mod, double water_delta, int use_limiter);
/* awm_add_mix_d for ONE span and n_payloads tables: out_d[p] (and, with a limiter, block_max_d[p]) receive what awm_add_mix_d writes
 * for the span with frame_mod[p], bit for bit.  The span is read, windowed and transformed forward once per pass of at most 4 outputs
 * (K2m's span form, hip/kernels.hip; passes are balanced: 5 payloads run as 3 + 2) -- the halo frames too.  Same rules as awm_add_mix_d:
 * the span starts on a frame boundary, every block_max_d[p] (n_blocks floats from block first_block) is pre-initialised with
 * awm_add_init_block_max_d, the outputs are limited one by one with awm_add_limit_d.  frame_mod: n_payloads host tables.
 * AWM_ERR_ARG with nothing enqueued: n_payloads == 0, a NULL pointer (block_max_d itself may be NULL: no limiter), an output that
 * overlaps the input, a halo or another output; with more than one payload also a call while the SNR meter is armed.
 * awm_debug_set_add_payloads_fused (0) makes it a loop over awm_add_mix_d. */
int awm_add_mix_payloads_d (awm_ctx *ctx, const float *pcm_in_d, float *const *out_d, size_t n_payloads, size_t n_frames, int n_channels,
                            const int8_t *const *frame_mod /* host, one per payload */, double water_delta, size_t first_frame,
                            const float *halo_before_d, const float *halo_after_d,
                            float *const *block_max_d /* NULL: no limiter; else n_payloads arrays */, size_t first_block, size_t n_blocks);

/* add as a tile loop with bounded memory -- the reference's streaming add_stream_watermark (wmadd.cc:520-589) keeps one
 * frame (WatermarkSynth, wmadd.cc:173,220-222) and up to two limiter blocks (limiter.cc:51-64) of state; here the unit in
 * flight is a tile of `tile_frames1024` frames (>= 128) and the same state is carried from tile to tile inside the object.
 *   create:  payload / key tables are resolved once (Params as at this call).
 *   input:   device pointer where the NEXT tile's interleaved float32 samples are to be written (tile_frames1024 * 1024 * C).
 *   push:    `n_frames` samples per channel were written there; every tile but the last must be full; last = 1 ends the
 *            stream (n_frames may be 0).  Work is enqueued on the context's stream.  Returns how many tiles became final
 *            (0..3, in stream order): out_d[i] / out_frames[i] point into the object and stay valid until the next push.
 * The concatenated output is bit-identical to awm_add_watermark_d on the whole stream (tests: spans + halo == whole).
 *   create_at: the `zero_frames` argument of add_stream_watermark (wmcommon.hh:226; wmadd.cc:501-526, 574-580, limiter.cc:69-88):
 *            the stream starts `zero_frames` samples into the frame / watermark block / limiter block grid, as if that many zeros
 *            had been pushed before the caller's first sample and cut from the output again.  Whole frames of zeros are only
 *            counted (the table row of frame m becomes (4202 + zero_frames / 1024 + m) mod 4452, the limiter blocks keep their
 *            phase); the remaining zero_frames % 1024 zeros sit in front of the caller's samples inside the object, so the
 *            LAST tile's output may be up to 1023 frames longer than its input was (what hung over the tile before it). */
typedef struct awm_add_stream awm_add_stream;
int    awm_add_stream_create (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, int n_channels, size_t tile_frames1024,
                              awm_add_stream **out);
int    awm_add_stream_create_at (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, int n_channels, size_t tile_frames1024,
                                 size_t zero_frames, awm_add_stream **out);
void   awm_add_stream_destroy (awm_add_stream *s);
float *awm_add_stream_input (awm_add_stream *s);
int    awm_add_stream_push (awm_add_stream *s, size_t n_frames, int last, const float *out_d[3], size_t out_frames[3]);
/* The tile loop for ONE input and n_payloads payloads (1 .. AWM_ADD_STREAM_MAX_PAYLOADS) with one key: the same object with three input
 * slots as before, three mix slots, a table and an array of block maxima PER PAYLOAD.  awm_add_stream_input / awm_add_stream_destroy are
 * unchanged; awm_add_stream_push_payloads pushes as awm_add_stream_push does (mix tile t - 1 once tile t is there -- one
 * awm_add_mix_payloads_d-like pass over the tile and its halos for all payloads --, limit tile t - 2 per output, flush on last) and returns
 * how many tiles became final: out_d has room for 3 * n_payloads pointers, out_d[i * n_payloads + p] is finished tile i of payload p,
 * out_frames[i] its length for every payload.  zero_frames as in awm_add_stream_create_at.  The concatenated output p is bit-identical to
 * an awm_add_stream with payload p.  HBM: (3 + 3 n_payloads) tiles.
 * AWM_ERR_ARG: n_payloads == 0 or > AWM_ADD_STREAM_MAX_PAYLOADS, a payload that does not parse (awm_last_error names its index),
 * awm_add_stream_push on an object with more than one payload, creating such an object -- or pushing to one with more than one payload --
 * while the SNR meter is armed.  awm_add_stream_push_payloads on a one-payload object is awm_add_stream_push. */
#define AWM_ADD_STREAM_MAX_PAYLOADS 64
int    awm_add_stream_create_payloads_at (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads,
                                          int n_channels, size_t tile_frames1024, size_t zero_frames, awm_add_stream **out);
size_t awm_add_stream_payloads (const awm_add_stream *s);        /* 0 for NULL */
int    awm_add_stream_push_payloads (awm_add_stream *s, size_t n_frames, int last,
                                     const float **out_d /* [3][n_payloads] */, size_t out_frames[3]);

/* The tile loop at ANY sample rate that zita's fixed-ratio Resampler takes in both directions (what awm_add_watermark_segments_rate_d takes;
 * DESIGN.md section 9.5): the same object, the same input / push / push_payloads / payloads / destroy calls and the same contract -- every
 * tile but the last full, last = 1 ends the stream, a push only enqueues on the context's stream (no host synchronise but for the growth of
 * the block maxima), 0 .. 3 finished tiles per push in stream order, tile t final no later than the push of tile t + 2, pointers valid
 * until the next push.  A tile is tile_frames1024 * 1024 samples per channel AT sample_rate, and output tiles have exactly the lengths of
 * the input tiles: every stage works at global sample and frame indices, so zero_frames needs no zeros inside the object.
 * With x = the concatenated input, output p is bit for bit what awm_add_watermark_d (ctx, key, payload_hex[p], x, ..., sample_rate) writes
 * for zero_frames == 0 and what awm_add_watermark_segments_rate_d writes for the single segment (zero_frames, x) otherwise; the end of the
 * stream need not be known, both see zeros behind it.  sample_rate == 44100 forwards to awm_add_stream_create_at /
 * awm_add_stream_create_payloads_at.
 * Per push: resample what arrived down to 44.1 kHz as far as the windows are filled (K10s: launches end on multiples of np, the rest is
 * carried), K2 / K2m for the watermark signal alone over the whole frames that became available (the last one is the halo), per payload
 * resample the complete frames up, mix + block maxima (in front of the stream the stretch of watermark alone that only counts for the
 * maxima), then the limiter for tile t - 2.  The number of launches of a push does not depend on the tiles before it.
 * HBM, reserved at creation (T = a tile, T44 = T * 44100 / sample_rate, both plus a few thousand samples of carry): 2 T input + 2 T44 at
 * 44.1 kHz + 2 n_payloads T44 watermark frames + 1 T watermark signal + 3 n_payloads T mix slots: (3 + 3 n_payloads) T + (2 + 2 n_payloads) T44;
 * (the context's allocator rounds every buffer up, by half at most); the block maxima (4 bytes per second and payload: the first 4096 with
 * the object) grow as before.
 * AWM_ERR_ARG, nothing allocated or enqueued: what the 44.1 kHz constructors refuse, sample_rate <= 0, a rate without a fixed-ratio table
 * in either direction (e.g. 44101), a tile below awm_add_stream_rate_plan's min_tile, creation or a push while the SNR meter is armed (the
 * powers of the resampled add are defined over the whole stream), a push that takes zero_frames + the samples pushed to 2^40 or beyond. */
int    awm_add_stream_create_rate_at (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, int n_channels, int sample_rate,
                                      size_t tile_frames1024, size_t zero_frames, awm_add_stream **out);
int    awm_add_stream_create_payloads_rate_at (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads,
                                               int n_channels, int sample_rate, size_t tile_frames1024, size_t zero_frames,
                                               awm_add_stream **out);
int    awm_add_stream_sample_rate (const awm_add_stream *s);      /* 44100 for the objects of the constructors above, 0 for NULL */
/* The look-ahead of that object (pure host arithmetic, no context, no device; the object calls it).  With b_X (m) = floor (m step_X / np_X):
 *   down_ahead: 44.1 kHz sample q reads the stream up to b_down (q) + down_ahead;
 *   mix_ahead:  the smallest L such that the mix of output sample m, for every m, depends on no input sample beyond m + L (up window ->
 *               frame of the last watermark sample read -> the frame after it -> its last 44.1 kHz sample -> that sample's down window);
 *   min_tile:   the smallest tile in samples for which tile t is final after the push of tile t + 2: one limiter block + mix_ahead,
 *               rounded up to 1024, and at least 128 * 1024.
 * 0, or AWM_ERR_ARG for a rate the object refuses. */
typedef struct { uint64_t limiter_block, down_ahead, mix_ahead, min_tile; int down_hl, down_np, down_step, up_hl, up_np, up_step; } awm_stream_rate_plan;
int    awm_add_stream_rate_plan (int sample_rate, awm_stream_rate_plan *plan);

/* I/O staging: RawConverter::from_raw / to_raw (rawconverter.cc:155-286) on the device, so that files cross PCIe in
 * their own sample format.  bit_depth 8/16/24/32 (integer) or 32/64 (float); encoding 0 signed, 1 unsigned, 2 float.
 * direct16 != 0 selects the reference's native little-endian signed-16 rule (truncate at 16 bit, what its stdout / raw
 * writers do); 0 = clip to 32 bit and keep the top bits (what writing through libsndfile does). */
int awm_pcm_decode_d (awm_ctx *ctx, const void *bytes_d, size_t n_values, int bit_depth, int encoding, int big_endian, float *out_d);
int awm_pcm_encode_d (awm_ctx *ctx, const float *in_d, size_t n_values, int bit_depth, int encoding, int big_endian, int direct16,
                      void *bytes_d);

/* SyncFinder::sync_fft (syncfinder.cc:560-605): dB magnitudes of bins 20..100, channels summed.
 * db_out_d: [frame_count][81] float32, have_out_d: [frame_count] bytes.
 * want_frames (host, may be NULL) and [first,last) (value indices of the non-silent range,
 * syncfinder.cc:155-169) reproduce the reference's skip rules. */
int awm_sync_fft_d (awm_ctx *ctx, const float *pcm_d, size_t n_frames, int n_channels,
                    size_t index, size_t frame_count, const char *want_frames,
                    size_t first, size_t last, float *db_out_d, char *have_out_d);

/* SyncFinder::search (syncfinder.cc:487-558) for one key: search_approx on the 4 shifts,
 * local mean, peak selection, search_refine, final selection.  Returns the number of scores
 * (<= max_out), sorted by index.  block_type: 0 = A, 1 = B. */
int awm_sync_search_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames,
                       int n_channels, int clip_mode, size_t max_out,
                       uint64_t *index, double *quality, int *block_type);
/* search_approx only (syncfinder.cc:171-256): all candidate scores in index order */
long awm_search_approx_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames,
                          int n_channels, int clip_mode, size_t max_out,
                          uint64_t *index, double *raw_quality, double *local_mean);

/* FFTAnalyzer::fft_range(index, 2226) + mix_decode (wmget.cc:67-108) for `n_blocks` block
 * start indices: raw soft bits in mix order, out[n_blocks][858].  ok[i] = 0 where the block
 * would read past the end (fft_range returns empty, wmcommon.cc:128-130). */
int awm_block_soft_bits_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames,
                           int n_channels, const uint64_t *index, size_t n_blocks, float *out, int *ok);

/* conv_decode_soft (convcode.cc:128-213) for a batch of equally typed blocks.
 * soft: [n][coded_len] normalised soft bits; bits_out: [n][coded_len/rate - 15]; error_out[n].
 * coded_len / rate = 15 ... 256 trellis steps (the termination alone up to 64 rounds of 4 steps); other lengths and a coded_len
 * that is no multiple of the rate (6 for A and B blocks, 12 for AB) return AWM_ERR_ARG before anything is launched. */
int awm_viterbi_decode (awm_ctx *ctx, int block_type, const float *soft, size_t coded_len, size_t n,
                        int *bits_out, float *error_out);

/* ---- pipeline level ------------------------------------------------------------------- */
typedef struct
{
  double   time;           /* seconds, incl. chunk offset */
  uint64_t sync_index;     /* sample index inside its chunk */
  double   sync_quality;
  int      block_type;     /* 0 A, 1 B, 2 AB */
  int      type;           /* 0 BLOCK, 1 CLIP, 2 ALL */
  float    decode_error;
  double   speed;
  int      bits[128];
  int      n_bits;
} awm_pattern;

/* add_watermark for n_clips independent inputs with one key and payload: what n_clips `audiowmark add` runs produce
 * (wmadd.cc:620-657), the clips dealt to the context's work lanes so that their small kernels overlap.  All clips at the
 * watermark rate (44100 Hz) with n_channels channels; out_d[i] holds n_frames[i] * n_channels floats. */
int awm_add_watermark_batch_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, size_t n_clips, const float *const *pcm_in_d,
                               float *const *out_d, const size_t *n_frames, int n_channels);

/* A batch of stream SEGMENTS with one key, each with its own offset and payload: what the reference's HLS mode does per request
 * (hls.cc:244-279: a few seconds of audio with up to 3 x 1024 samples of context on either side, watermarked for one subscriber by
 * add_stream_watermark (key, in, out, bits, start_pos - prev_size), hls.cc:279).  For every i, out_d[i] receives n_frames[i] * n_channels
 * floats: bit for bit the concatenated output of an awm_add_stream_create_at (ctx, key, payload_hex[i], n_channels, ..., zero_frames[i])
 * stream fed that segment.  44100 Hz (other rates: awm_add_watermark_segments_rate_d below); the context's parameters apply as for awm_add_watermark_d
 * (water_delta, mix, frames_per_bit, test_no_limiter).  Inputs may alias each other (the same segment for many subscribers).
 * AWM_ERR_ARG with nothing enqueued: a NULL pointer (pcm_in_d[i] / out_d[i] may be NULL where n_frames[i] is 0), an output that overlaps
 * an input or another output, a payload that does not parse (awm_last_error names its index), a call while the SNR meter is armed.
 * n_segments == 0 returns 0; a segment with n_frames == 0 writes nothing.
 * Stereo, 16-byte aligned pointers and n_segments >= 2 take the fused path: the batched clip machine (one launch per stage, blockIdx.y =
 * segment; the number of launches does not depend on n_segments up to the 4096 segments a launch takes) with, per segment, its place in
 * the frame and limiter grids (first_frame = zero_frames / 1024, limiter phase and block from zero_frames) and the table of its payload.
 * No table is built on the host: K16p (hip/keytab.hip) expands the key's template (awm_tab_frame_mod_template, cached per context) with
 * the payloads' codes, one launch per group of at most 1024 DISTINCT payloads; equal payload strings share a table; the host contributes
 * parse_payload + conv_encode per distinct payload.  A segment with r = zero_frames % 1024 != 0 begins r samples into its first frame:
 * such segments are staged -- one gather launch per batch writes "r zeros, then the segment" into aligned slices of a workspace, K2 and
 * the limiter work there, one scatter launch brings the results home without the r samples (a batch stages at most 1 GiB per direction,
 * more is split); segments with r = 0 are read from and written to the caller's buffers directly.  Everything else (other channel
 * counts, a misaligned pointer, a single segment, awm_debug_set_add_batched (0)) goes segment by segment through the tile stream, with
 * the same results.  Not offered in this form: the command line, the awm_multi_* / sharded forms.  A key per segment:
 * awm_add_watermark_segments_keys_d below. */
int awm_add_watermark_segments_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex,
                                  const size_t *zero_frames, const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames,
                                  int n_channels);

/* The same at ANY sample rate that zita's fixed-ratio Resampler takes in both directions (48000, 32000, 96000, 22050, 88200, ...: what the
 * reference's HLS mode does with add_stream_watermark at the rate of the programme, WatermarkResampler, wmadd.cc:353-430).  With S = the
 * stream "zero_frames[i] zeros, then segment i" and W = what awm_add_watermark_d (ctx, key, payload_hex[i], S, W, zero_frames[i] +
 * n_frames[i], n_channels, sample_rate) writes, out_d[i] receives W[zero_frames[i] ... zero_frames[i] + n_frames[i]), bit for bit -- but
 * no zero is ever stored and nothing is computed outside a WINDOW of a few 44.1 kHz frames around the segment (awm_add_segment_plan): every
 * stage of the resampled add is a function of global sample and frame indices.  The cost does not depend on zero_frames.
 * Arguments and rules are awm_add_watermark_segments_d's (AWM_ERR_ARG with nothing enqueued, the overlap sweep, aliasing inputs, the payload
 * index in the error, refused while the SNR meter is armed, n_segments == 0 and empty segments accepted; the context's water_delta, mix,
 * frames_per_bit, test_no_limiter apply); sample_rate == 44100 IS that function.  Refused in addition, with AWM_ERR_ARG and nothing written:
 * sample_rate <= 0, a rate without a fixed-ratio table in either direction (e.g. 44101: the reference would use zita's VResampler there,
 * which this entry point does not offer), zero_frames[i] + n_frames[i] >= 2^40.
 * Stereo, 16-byte aligned pointers, n_segments >= 2 (and a rate of at least 8192 Hz) take the fused path, per batch: [K16p], K10w down
 * (blockIdx.y = slice; segments that agree in pcm_in_d, n_frames and zero_frames share ONE 44.1 kHz slice), fill, K2 (watermark signal
 * alone, per segment), K10w up, mix + block maxima, K3a, K3b -- the number of launches does not depend on n_segments up to the 4096 a launch
 * takes; the 44.1 kHz slices and the watermark signals live in three context workspaces of at most 1 GiB each, larger batches are split.
 * Everything else (other channel counts, a misaligned pointer, a single segment, awm_debug_set_add_batched (0), a call with a segment
 * whose window alone exceeds such a workspace: about 50 minutes of stereo) runs the same stages segment by segment with the same window
 * arguments and the same results; awm_debug_add_segments_fused_in_use () tells which path ran.
 * Not offered in this form: the command line, the awm_multi_* / sharded forms.  A key per segment: awm_add_watermark_segments_keys_rate_d
 * below. */
int awm_add_watermark_segments_rate_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex,
                                       const size_t *zero_frames, const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames,
                                       int n_channels, int sample_rate);

/* The same two with a KEY PER SEGMENT (a service that carries several programmes or tenants, a key each, in one queue): keys = n_segments x
 * 16 bytes in host memory, and out_d[i] is bit for bit what awm_add_watermark_segments_d (at a rate: awm_add_watermark_segments_rate_d)
 * writes for segment i alone with keys + 16 i.  Arguments, refusals with nothing enqueued (NULL pointers, the overlap sweep, a payload that
 * does not parse with its index in awm_last_error, the SNR meter; at a rate: the rate and 2^40), aliasing inputs, empty segments and
 * sample_rate == 44100 are those functions'; in addition keys == NULL with n_segments > 0 is AWM_ERR_ARG.  A call whose segments all
 * carry one key IS the one-key function.
 * The fused path (stereo, 16-byte aligned pointers, n_segments >= 2) orders the segments by (key, payload); equal pairs share a table.  The
 * host contributes the 176-byte AES key schedule per distinct key and parse_payload + conv_encode per distinct payload: no table and,
 * at the default geometry, no template is built on the host.  Per table group of at most 1024 distinct pairs, K16t (hip/keytab.hip) builds
 * the templates of the keys the group needs and that an earlier group has not left behind -- one workgroup per key, at most 256 keys per
 * launch --, K16p expands every pair's table from its key's template in one launch, and the stages of the one-key path run unchanged
 * (at a rate, segments that agree in input, length and offset still share their 44.1 kHz slice whatever their keys).  At fixed numbers of
 * distinct keys and pairs the number of launches does not depend on n_segments.  The templates (721 KB per key, at most 1024 slots) and
 * K16t's scratch live in grow-only context workspaces that awm_ctx_trim gives back.  Other geometries (mix off, frames_per_bit != 2,
 * another payload size) and awm_debug_set_key_tables_on_device (0) take the host's templates through the context's cache, one copy per
 * key, with the same results.  Everything the fused path does not take goes segment by segment through the one-key per-segment path with
 * that segment's key; awm_debug_add_segments_fused_in_use () tells which path ran.
 * Not offered in this form: the command line, the file level, the awm_multi_* / sharded forms. */
int awm_add_watermark_segments_keys_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex,
                                       const size_t *zero_frames, const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames,
                                       int n_channels);
int awm_add_watermark_segments_keys_rate_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex,
                                            const size_t *zero_frames, const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames,
                                            int n_channels, int sample_rate);
/* The segment batches FROM AND TO SIGNED 16-BIT PCM (little-endian, interleaved: what a decoder hands out and an encoder takes back, the
 * reference's native rule, rawconverter.cc:197-198) -- no float copy of a segment that the caller can see, no decode or encode launch
 * per segment.  Segment i = n_frames[i] frames of n_channels int16 values at pcm_in_d[i]; out_d[i] receives as many.  sample_rate == 44100
 * is the 44.1 kHz form (there are no symbols of their own for it).
 * Definition: with f_i = what awm_pcm_decode_d (ctx, pcm_in_d[i], n_frames[i] * n_channels, 16, 0, 0, f_i) writes and g_i = what
 * awm_add_watermark_segments_rate_d (the keys form: awm_add_watermark_segments_keys_rate_d, with keys + 16 i) writes for segment i on the
 * inputs f_i, out_d[i] is value for value what awm_pcm_encode_d (ctx, g_i, n, 16, 0, 0, 1, out_d[i]) writes: v * 32768, saturated at 32767
 * and -32768, truncated.
 * Rules: those of the float functions -- AWM_ERR_ARG with nothing enqueued and nothing written, the index of the offending segment in
 * awm_last_error, aliasing inputs, empty segments and n_segments == 0 accepted, refused while the SNR meter is armed, the rate and 2^40, the
 * context's water_delta, mix, frames_per_bit and test_no_limiter, keys == NULL, one key for all segments IS the one-key call.  The overlap
 * sweep works on the byte ranges of n C 2 bytes; a pcm_in_d[i] or out_d[i] at an odd address is refused.  Pointers need only 2-byte
 * alignment, and nothing outside [out_d[i], out_d[i] + n C) is written.
 * The fused paths take stereo, n_segments >= 2 and every pointer 4-byte aligned (a stereo frame is one load or store; at a rate: at least
 * 8192 Hz).  The float intermediates are the context's batch workspaces of the float paths and nothing else, and the number of launches
 * does not depend on n_segments.  At a rate: K10w down READS THE 16-BIT VALUES (the kernel instantiated for 16-bit input: a value is
 * converted once, where it leaves global memory; segments that agree in input, length and offset share one slice), K2 and K10w up are
 * unchanged, the block maxima come from decode (in) + wm without a stored mix, and one last kernel computes that sum again, scales by the
 * limiter's ramp, encodes and stores int16 to out_d.  At 44.1 kHz: one gather decodes every segment into its staged slice ("r zeros, then
 * the segment", the r == 0 segments too), K2 and the limiter's table run there, and the limiter's apply pass with a 16-bit sink reads the
 * un-limited mix behind the r samples, scales, encodes and stores to out_d.
 * Everything else (other channel counts, a pointer that is only 2-byte aligned, a single segment, awm_debug_set_add_batched (0), at a rate a
 * segment whose window exceeds a workspace) goes segment by segment through the definition: decode into a context workspace, the float
 * path of one segment, encode into out_d[i]; awm_ctx_trim gives the workspace back, awm_debug_add_segments_fused_in_use () tells which path
 * ran.
 * Not offered in this form: other sample formats, `add` batches of whole clips, the tile stream, the command line, the file level (which
 * converts its files' formats itself), the awm_multi_* / sharded forms. */
int awm_add_watermark_segments_rate_s16_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex,
                                           const size_t *zero_frames, const int16_t *const *pcm_in_d, int16_t *const *out_d,
                                           const size_t *n_frames, int n_channels, int sample_rate);
int awm_add_watermark_segments_keys_rate_s16_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex,
                                                const size_t *zero_frames, const int16_t *const *pcm_in_d, int16_t *const *out_d,
                                                const size_t *n_frames, int n_channels, int sample_rate);
/* The segment batches WITH A SAMPLE RATE PER SEGMENT: a request queue that is not sorted by rate in one call.  Each
 * function is its _rate counterpart above with sample_rates (host, one rate per segment) in place of sample_rate.
 * Definition: out_d[i] is bit for bit (16-bit: value for value) what the one-rate function of the same family writes for segment i alone
 * at sample_rates[i]; the keys forms use keys + 16 i there.
 * A call whose rates are all equal IS the one-rate function and forwards before anything else (all 44100: the 44.1 kHz function); one key
 * for all segments of a keys form IS the one-key form.  sample_rates == NULL: the float forms refuse it when n_segments > 0 (AWM_ERR_ARG,
 * like awm_get_watermark_batch_rates_d), the 16-bit forms take every segment at 44100 (like awm_get_watermark_batch_rates_s16_d).
 * Rules: those of the one-rate functions -- AWM_ERR_ARG with nothing enqueued and nothing written, the index of the first offending segment
 * in awm_last_error, for a sample_rates[i] <= 0, a rate without a fixed-ratio table in both directions, zero_frames[i] + n_frames[i] >= 2^40
 * at that segment's rate, NULL pointers, the overlap sweep (16-bit: n C 2 bytes, odd addresses), a payload that does not parse, an armed SNR
 * meter, keys == NULL.  n_segments == 0 returns 0, empty segments write nothing, the rate of an empty segment is still checked.
 * The fused path takes stereo, n_segments >= 2, every pointer aligned as the one-rate fused paths need it (float 16-byte, 16-bit 4-byte),
 * every rate other than 44100 at least 8192 Hz and with windows that fit a workspace, awm_debug_set_add_batched on.  It is one upload and one
 * chain of launches: the batches are not split by rate -- K10w, the mix / maxima kernels, the batched limiter and the 16-bit encode pass
 * read the resampler's geometry and the limiter block from each segment's descriptor --, segments share a down-resampled slice only if they
 * agree in input, length, offset and rate, the segments at 44100 run the stages of the 44.1 kHz fused path as a sub-batch of the same call,
 * and all of them read the same tables: K16p runs once per table group, K16t once per key, however many rates the call holds.  No workspace
 * beyond those of the one-rate paths; awm_ctx_trim gives everything back.
 * Everything else goes segment by segment through the one-rate path of one segment at that segment's rate;
 * awm_debug_add_segments_fused_in_use () tells which path ran.
 * Not offered: the command line, the file level, the tile stream, the awm_multi_* / sharded forms. */
int awm_add_watermark_segments_rates_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex,
                                        const size_t *zero_frames, const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames,
                                        int n_channels, const int *sample_rates);
int awm_add_watermark_segments_keys_rates_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex,
                                             const size_t *zero_frames, const float *const *pcm_in_d, float *const *out_d,
                                             const size_t *n_frames, int n_channels, const int *sample_rates);
int awm_add_watermark_segments_rates_s16_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex,
                                            const size_t *zero_frames, const int16_t *const *pcm_in_d, int16_t *const *out_d,
                                            const size_t *n_frames, int n_channels, const int *sample_rates);
int awm_add_watermark_segments_keys_rates_s16_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex,
                                                 const size_t *zero_frames, const int16_t *const *pcm_in_d, int16_t *const *out_d,
                                                 const size_t *n_frames, int n_channels, const int *sample_rates);
/* The window of one such segment (pure host arithmetic, no context, no device; the device path calls it per segment).  Frames and samples
 * are indices into the segment's stream: at 44.1 kHz for the frames (of 1024 samples) and the down_* samples, at sample_rate otherwise. */
typedef struct
{
  uint64_t mix_first;                /* first sample of the stream whose mix counts: the watermark begins this far in front of zero_frames
                                        (resampler pre-ringing, the frames that see the segment's first sample); it is needed only for the
                                        limiter's block maxima */
  uint64_t frame_first, frame_last;  /* 44.1 kHz frames K2 must produce completely (those the up-resampler reads) */
  uint64_t slice_first, slice_last;  /* frames K2 runs over: one more on either side, transformed but incomplete (none in front of frame 0) */
  uint64_t down_first, down_last;    /* 44.1 kHz samples the down-resampler must deliver: those of the slice's frames */
  uint64_t in_first, in_last;        /* samples of the segment (relative to it) those depend on */
  uint64_t limiter_block;            /* samples per limiter block at sample_rate */
  uint64_t first_block, n_blocks;    /* limiter blocks whose maxima are kept: from the block of mix_first */
  int      down_hl, down_np, down_step, up_hl, up_np, up_step;     /* the two resamplers' tables (kernels.hh ResampleArgs) */
} awm_segment_plan;
/* 0, or AWM_ERR_ARG for what awm_add_watermark_segments_rate_d refuses (rate, 2^40).  n_frames == 0: only the tables and limiter_block */
int awm_add_segment_plan (int sample_rate, size_t zero_frames, size_t n_frames, awm_segment_plan *plan);

/* The batch entry points with ONE KEY PER CLIP (keys = n_clips * 16 bytes; BASELINE configs[4]: `--test-key k` for clip k).  The key
 * tables -- frame_mod for `add`; CLIP sync tables, mix table and bit order for `get` (wmcommon.cc:143-202, wmadd.cc:86-162,
 * syncfinder.cc:30-77) -- are built group by group while the device works on the previous group and are indexed per clip inside the
 * group's launches: `add`'s frame_mod tables ON THE DEVICE (K16, hip/keytab.hip: AES-128-CTR streams and the shuffles of one key
 * per workgroup, 256 keys per launch; the host contributes the AES key schedules, 176 bytes per key), `get`'s tables on host
 * threads, 64 clips per group, one copy per group.  Results per clip equal awm_add_watermark_d / awm_get_watermark_d with that
 * clip's key. */
int awm_add_watermark_batch_keys_d (awm_ctx *ctx, const uint8_t *keys, const char *payload_hex, size_t n_clips, const float *const *pcm_in_d,
                                    float *const *out_d, const size_t *n_frames, int n_channels);
int awm_get_watermark_batch_keys_d (awm_ctx *ctx, const uint8_t *keys, size_t n_clips, const float *const *pcm_d,
                                    const size_t *n_frames, int n_channels, int n_threads, size_t max_out_per_clip,
                                    awm_pattern *out, int *n_out);

/* add_watermark core (wmadd.cc:448-618) on resident PCM: out_d gets n_frames*C samples.  AWM_ERR_ARG with nothing enqueued if out_d
 * overlaps pcm_in_d anywhere (every output frame is computed from three input frames: an overlap would be a race). */
int awm_add_watermark_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex,
                         const float *pcm_in_d, float *out_d, size_t n_frames, int n_channels,
                         int sample_rate);
/* add_watermark (wmadd.cc:448-618) of ONE input with n_payloads payloads and one key: out_d[p] receives what
 * awm_add_watermark_d (ctx, key, payload_hex[p], pcm_in_d, out_d[p], ...) would write, bit for bit -- the same programme for many
 * recipients, each copy with a payload of its own (what the reference prepares once and then marks per subscriber in its HLS mode,
 * hls.cc).  The frame_mod tables of two payloads differ only in UP <-> DOWN of the data frames' bands (mark_data, wmadd.cc:86-162), so at
 * 44100 Hz one kernel (K2m, hip/kernels.hip) reads, windows and transforms every frame once and computes both band factors once; the
 * choice per band, the inverse transform, overlap-add, mix, block maxima and limiter run per output, ADD_MULTI_TILE (4) outputs per pass
 * over the input.  Every channel count takes the fused kernel (stereo with both channels in a wave, anything else a channel per wave).
 * At another sample rate with fixed-ratio tables both ways (48, 32, 96, 22.05, 88.2 kHz ...) the payload-independent work of the resampled
 * add is shared as well: the stream goes down to 44.1 kHz once per call, K2m writes the watermark signals of a pass
 * alone, and per pass they go up to the rate and into the outputs -- stereo at 48 kHz with 8-byte aligned pointers in one kernel (K10m:
 * up-resample, add the input, block maxima), everything else through K10 and K11 once per output; the limiter per output.  Workspaces: the
 * 44.1 kHz stream and min (n_payloads, 4) watermark signals of its size, 6.4 GB for 60 min of stereo at 48 kHz (the loop: 3.9 GB); if they
 * cannot be reserved the call frees them and loops.  Rates that only the VResampler takes (44101 Hz) loop over the single-payload path.
 * The context's parameters apply as for awm_add_watermark_d.  n_payloads == 0 or n_frames == 0: returns 0, writes nothing; n_payloads == 1: the single-payload path.
 * AWM_ERR_ARG with nothing enqueued: a payload that does not parse (awm_last_error names its index), a NULL pointer, an output that
 * overlaps the input or another output, a call while the SNR meter is armed (awm_ctx_snr_begin).
 * The same for a span of a stream: awm_add_mix_payloads_d; with bounded memory: awm_add_stream_create_payloads_at; for files:
 * awm_add_watermark_payloads_file.  Not offered in this form: the command line, sharding, a key per payload. */
int awm_add_watermark_payloads_d (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads,
                                  const float *pcm_in_d, float *const *out_d, size_t n_frames, int n_channels, int sample_rate);
/* Streams at another sample rate.  The reference resamples them to 44.1 kHz with zita-resampler (hlen 16): the fixed-ratio
 * Resampler where it takes the two rates, else the VResampler with ratio new / old (ResamplerImpl::create,
 * resample.cc:233-270).  `get` decodes the resampled stream (WavChunkLoader, wavchunkloader.cc:70-71,200-216), `add` generates the
 * watermark at 44.1 kHz and resamples the watermark signal back (WatermarkResampler, wmadd.cc:353-430) -- the latter is
 * what awm_add_watermark_d does for sample_rate != 44100.  awm_resample_d is the former: out_d receives n_out_frames
 * frames of the stream the reference's loader would hand to the decoder, awm_resample_frames tells how many there are
 * (0: neither zita class takes the ratio, i.e. it is below 1 / 16 or above 256).  zita-resampler is not part of the reference
 * tree; its algorithm is restated from the library's description, bit parity with it is unpinned. */
size_t awm_resample_frames (awm_ctx *ctx, size_t n_frames, int rate_in, int rate_out);
int awm_resample_d (awm_ctx *ctx, const float *pcm_in_d, size_t n_frames, int n_channels, int rate_in, int rate_out,
                    float *out_d, size_t n_out_frames);
/* get_watermark core (wmget.cc:886-1013) on resident 44.1 kHz PCM: chunk loop, BlockDecoder,
 * ClipDecoder, merge + sort.  Returns the pattern count (<= max_out filled). */
int awm_get_watermark_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames,
                         int n_channels, size_t max_out, awm_pattern *out);
/* add_watermark followed by get_watermark of its output, one key ("watermark, then verify that the payload decodes": wmadd.cc:448-618
 * then wmget.cc:886-1013, the two commands the reference runs one after the other in its own tests, tests/block-decoder-test.sh:8-18).
 * out_d receives the watermarked stream (pcm_in_d != out_d), `out` the pattern list of `get` on it: exactly what
 * awm_add_watermark_d + awm_get_watermark_d return.  As ONE call the library owns the order of the two halves on the context's stream:
 * `get` starts a chunk as soon as the limiter has passed the chunk's last sample instead of behind the whole `add` (two separate calls
 * cannot: the caller may have queued other work on the buffer in between).  Returns the pattern count or an error code. */
int awm_add_get_watermark_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const float *pcm_in_d, float *out_d,
                             size_t n_frames, int n_channels, int sample_rate, size_t max_out, awm_pattern *out);
/* WHOLE STREAMS FROM AND TO SIGNED 16-BIT PCM (little-endian, interleaved): `add`, and "watermark, then verify", on the 16-bit original
 * (DESIGN.md section 9.10).  pcm_in_d = n_frames frames of n_channels int16 values, out_d the same (device pointers).
 * Definition: with f = what awm_pcm_decode_d (ctx, pcm_in_d, n C, 16, 0, 0, f) writes -- float (v) * (1 / 32768), exact -- and g = what
 * awm_add_watermark_d writes for f, awm_add_watermark_s16_d writes to out_d, value for value, what awm_pcm_encode_d (ctx, g, n C, 16, 0, 0,
 * 1, out_d) writes: v * 32768, saturated at 32767 and -32768, truncated (the reference's native rule, rawconverter.cc:197-198).
 * awm_add_get_watermark_s16_d writes the same out_d and returns what awm_get_watermark_rate_s16_d returns on it, field for field; at
 * 44.1 kHz with the hand-over of awm_add_get_watermark_d: `get` starts a chunk once the last pass has passed the chunk's end.
 * The context's parameters apply as for awm_add_watermark_d (test_no_limiter, water_delta, frames_per_bit, the SNR meter).
 * Paths.  At 44.1 kHz, every channel count and any even address: K2 reads the int16 values itself (converted where they leave global
 * memory) and writes the un-limited float mix into a grow-only workspace of the context (n C 4 bytes, given back by awm_ctx_trim); one
 * last pass applies the limiter's ramp, encodes and stores int16 -- two passes, 12 bytes per value, no decode and no encode launch.
 * At a rate the fixed-ratio resampler takes both ways (48, 32, 96, 22.05, 88.2 kHz ...), stereo with both pointers 4-byte aligned and a
 * limiter block of at least 8192 samples: the down-resampler reads the int16 values, K2 writes the watermark signal alone, the
 * up-resampler brings it to the rate, the block maxima come from decode (in) + wm without a stored mix, and the last pass computes that
 * sum again, applies the ramp, encodes and stores.  Everything else (mono or three channels at a rate, 2-byte-only addresses at a rate,
 * rates that only the VResampler takes such as 44101, a call at a rate while the SNR meter is armed) goes through the definition on the context's
 * stream: decode into a float workspace, awm_add_watermark_d into a second one, encode into out_d; awm_ctx_trim gives both back.
 * awm_debug_add_s16_fused_in_use () tells which path ran.
 * out_d == pcm_in_d exactly is allowed: at 44.1 kHz the input has been consumed before the first int16 is stored; at a rate a frame of
 * the input is read for the last time by the thread that overwrites it.  n_frames == 0 returns 0 and writes nothing.
 * AWM_ERR_ARG with nothing enqueued and the outputs untouched: a NULL pointer with n_frames > 0, n_channels < 1, an int16 pointer at an
 * odd address, a payload that does not parse, a rate that neither zita class takes, an output that overlaps the input partially, and
 * (awm_add_get_watermark_s16_d) max_out > 0 with out == NULL.
 * Not offered from 16-bit input: many payloads (awm_add_watermark_payloads_d), the clip batches (awm_add_watermark_batch*_d), the tile
 * stream, the file level and the command line, the sharded and awm_multi_* forms, other sample formats. */
int awm_add_watermark_s16_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const int16_t *pcm_in_d, int16_t *out_d,
                             size_t n_frames, int n_channels, int sample_rate);
int awm_add_get_watermark_s16_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const int16_t *pcm_in_d, int16_t *out_d,
                                 size_t n_frames, int n_channels, int sample_rate, size_t max_out, awm_pattern *out);
/* The reference's get_watermark takes a LIST of keys (wmcommon.hh:228, `--key a --key b`, tests/key-test.sh:13-37): the file is
 * read once, the approximate dB matrices of a chunk / of a padded clip are computed once and shared by the keys
 * (syncfinder.cc:171-256), patterns are sorted by time with the key list order breaking ties (wmget.cc:288-316).
 * keys = n_keys * 16 bytes; key_of_pattern[j] (may be NULL) = position in that list of the key pattern j was found with. */
int awm_get_watermark_keys_d (awm_ctx *ctx, const uint8_t *keys, int n_keys, const float *pcm_d, size_t n_frames, int n_channels,
                              size_t max_out, awm_pattern *out, int *key_of_pattern);
/* get_watermark for a batch of independent inputs (BASELINE config 5: many short clips; the reference would run one
 * `audiowmark get` process per file, wmget.cc:886-1013 each).  Clip i = n_frames[i] frames at pcm_d[i] (device pointers),
 * all with n_channels channels.  Clips shorter than one block + 2 frames (51.7 s: only the ClipDecoder's START pass has work,
 * wmget.cc:769-884) are processed in groups of 64 whose padded copies lie side by side in one buffer -- every stage of the CLIP
 * search and of the decode is one launch per group; longer clips are spread over the context's work lanes (n_threads host
 * threads, <= 0: all lanes).  Patterns of clip i go to out[i * max_out_per_clip ...], their number (possibly >
 * max_out_per_clip) to n_out[i]; every clip's result equals awm_get_watermark_d on it.  Returns 0 or an error code. */
int awm_get_watermark_batch_d (awm_ctx *ctx, const uint8_t key[16], size_t n_clips, const float *const *pcm_d,
                               const size_t *n_frames, int n_channels, int n_threads, size_t max_out_per_clip,
                               awm_pattern *out, int *n_out);
/* The device-pointer `get` for material at ANOTHER SAMPLE RATE (HLS and video audio: 48 kHz): what the reference's loader does in front
 * of the decoder (WavChunkLoader resamples every chunk to 44.1 kHz, wavchunkloader.cc:70-71, 200-216), for one resident stream, a batch
 * of clips, and a batch with a key per clip.  Definition: with y_i = what awm_resample_d (clip i, sample_rate -> 44100) writes,
 * awm_resample_frames (n_frames[i], sample_rate, 44100) frames, the result for clip i is field for field what awm_get_watermark_d returns
 * for y_i (sync_index is an index into the 44.1 kHz stream, as in the reference) -- with that clip's key in the keys form.  One rate per
 * call.  A clip is short (the grouped path of awm_get_watermark_batch_d) by its 44.1 kHz length.  Short clips at a rate of the fixed-ratio
 * Resampler are resampled STRAIGHT INTO the group's padded slices (stage 0 of the group, one launch per group: no resampled copies, no launch per clip,
 * no second read); long clips, VResampler rates and calls with a speed parameter set resample each clip into a grow-only workspace of its
 * lane first (awm_ctx_trim gives these back).  sample_rate == 44100 is the existing function.  AWM_ERR_ARG with nothing enqueued and n_out
 * untouched: sample_rate <= 0, or a ratio that neither zita class takes (awm_resample_frames gives 0).  Empty clips: n_out[i] = 0.
 * Not offered in this form: the sharded / multi-context batches.  A rate per clip: awm_get_watermark_batch_rates_d below. */
int awm_get_watermark_rate_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels,
                              int sample_rate, size_t max_out, awm_pattern *out);
int awm_get_watermark_batch_rate_d (awm_ctx *ctx, const uint8_t key[16], size_t n_clips, const float *const *pcm_d,
                                    const size_t *n_frames, int n_channels, int sample_rate, int n_threads,
                                    size_t max_out_per_clip, awm_pattern *out, int *n_out);
int awm_get_watermark_batch_keys_rate_d (awm_ctx *ctx, const uint8_t *keys, size_t n_clips, const float *const *pcm_d,
                                         const size_t *n_frames, int n_channels, int sample_rate, int n_threads,
                                         size_t max_out_per_clip, awm_pattern *out, int *n_out);
/* The batches with a SAMPLE RATE PER CLIP: a detection queue is not sorted by rate (uploads and monitored programmes at 44.1, 48, 32, 22.05,
 * 88.2 and 96 kHz side by side), and one call per rate leaves every rate's last group of 64 underfilled.  Clip i is at sample_rates[i].
 * Definition: the result for clip i is field for field what awm_get_watermark_rate_d (ctx, key_i, pcm_d[i], n_frames[i], n_channels,
 * sample_rates[i], ...) returns -- awm_get_watermark_d on awm_resample_d (clip i, sample_rates[i] -> 44100), and on the clip itself where its
 * rate is 44100; key_i = key, or keys + 16 i in the keys form; sync_index counts 44.1 kHz samples.
 * Paths: a clip is short by its 44.1 kHz length.  Short clips at 44100 or at a rate of the fixed-ratio Resampler fill the groups of 64 in
 * call order WHATEVER THEIR RATES; stage 0 of a group whose clips do not share one rate is the same launcher (every clip resampled with its own
 * rate's table, or copied, straight into its padded slice: one launch per form present in the group, not per clip or rate), a group that
 * happens to share one rate runs as in the one-rate call.  Long clips, VResampler rates and 44.1 kHz long clips go over the work lanes, each
 * resampled with its own rate into its lane's grow-only workspace first; so does every clip while a speed parameter is set (one clip
 * per lane and host thread, in parallel, each with the one-clip speed search; awm_debug_set_speed_batch).  A call
 * whose rates are all equal IS the one-rate function above (44100: the 44.1 kHz function).
 * Refusals, AWM_ERR_ARG with nothing enqueued and n_out / out untouched, awm_last_error names the index of the first offending clip:
 * sample_rates NULL with n_clips > 0, a sample_rates[i] <= 0, a ratio that neither zita class takes (awm_resample_frames gives 0 for a
 * non-empty clip).  n_clips == 0 returns 0; an empty clip gives n_out[i] = 0.
 * Not offered in this form: the command line, the file level, the awm_multi_* / sharded batches. */
int awm_get_watermark_batch_rates_d (awm_ctx *ctx, const uint8_t key[16], size_t n_clips, const float *const *pcm_d,
                                     const size_t *n_frames, int n_channels, const int *sample_rates, int n_threads,
                                     size_t max_out_per_clip, awm_pattern *out, int *n_out);
int awm_get_watermark_batch_keys_rates_d (awm_ctx *ctx, const uint8_t *keys, size_t n_clips, const float *const *pcm_d,
                                          const size_t *n_frames, int n_channels, const int *sample_rates, int n_threads,
                                          size_t max_out_per_clip, awm_pattern *out, int *n_out);
/* Pure host, no context, no device: which way clip i of such a call goes -- path_out[i] = 0 a group | 1 a lane, fixed-ratio resampler (or
 * a long clip at 44100, which is not resampled) | 2 a lane, VResampler | 3 empty, nothing to do -- and its length at 44.1 kHz, with the
 * parameters in force (the short / long border is block frames + 2).  Either output may be NULL.  AWM_ERR_ARG for the rates that the calls
 * above refuse, with -1 in that clip's path_out (the other clips are still filled in).  The 16-bit batches below take the same paths:
 * the sample format does not change them. */
int awm_get_batch_rates_plan (size_t n_clips, const size_t *n_frames, const int *sample_rates, int *path_out, size_t *n44_out);
/* The batches with a rate per clip on clips that are resident as SIGNED 16-BIT PCM (little-endian, interleaved: what a decoder or a capture
 * card hands out, the reference's native rule, rawconverter.cc) -- no float copy of a clip beside or instead of its 16-bit original, no
 * decode launch per clip.  Clip i = n_frames[i] frames of n_channels int16 values at pcm_d[i] (device pointers), at sample_rates[i];
 * sample_rates == NULL: every clip is at 44100.
 * Definition: with f_i = what awm_pcm_decode_d (ctx, pcm_d[i], n_frames[i] * n_channels, 16, 0, 0, f_i) writes -- float (v) * (1 / 32768),
 * exact -- the result for clip i is field for field what awm_get_watermark_batch_rates_d returns for f_i at sample_rates[i]; key_i = key, or
 * keys + 16 i in the keys form.
 * Paths: those of awm_get_watermark_batch_rates_d (awm_get_batch_rates_plan).  Stage 0 of a group of short clips READS THE 16-BIT VALUES:
 * the copy and the resampling forms are the same kernels instantiated for 16-bit input, which convert where a value leaves global memory (once per
 * input value) and are bit for bit the float kernels on f_i behind that; a short clip never has a float copy and never costs a launch of
 * its own.  Long clips, VResampler rates and every clip while a speed parameter is set are decoded into a grow-only workspace of their lane
 * first (one launch; awm_ctx_trim gives it back) and go on as in the float call.
 * Alignment: pcm_d[i] need only be 2-byte aligned.  A stereo group whose resampled clips are all 4-byte aligned loads whole frames
 * and keeps the phase-per-thread form for 48 kHz; one clip on an address that is only 2-byte aligned sends its group to the generic taps
 * (same bits).  Nothing outside a clip's values is read.
 * Refusals, AWM_ERR_ARG with nothing enqueued and n_out / out untouched, awm_last_error names the index of the first offending clip:
 * those of awm_get_watermark_batch_rates_d for the rates (except that sample_rates may be NULL), an odd pcm_d[i], a NULL pcm_d[i] with
 * n_frames[i] > 0.  n_clips == 0 returns 0; an empty clip gives n_out[i] = 0.
 * Not offered in this form: other sample formats, a format per clip, the command line, the file level (which converts its files' formats
 * itself), the awm_multi_* / sharded batches.  The `add` side: awm_add_watermark_segments_rate_s16_d, for the segment batches. */
int awm_get_watermark_batch_rates_s16_d (awm_ctx *ctx, const uint8_t key[16], size_t n_clips, const int16_t *const *pcm_d,
                                         const size_t *n_frames, int n_channels, const int *sample_rates, int n_threads,
                                         size_t max_out_per_clip, awm_pattern *out, int *n_out);
int awm_get_watermark_batch_keys_rates_s16_d (awm_ctx *ctx, const uint8_t *keys, size_t n_clips, const int16_t *const *pcm_d,
                                              const size_t *n_frames, int n_channels, const int *sample_rates, int n_threads,
                                              size_t max_out_per_clip, awm_pattern *out, int *n_out);
/* WHOLE STREAMS resident as SIGNED 16-BIT PCM (little-endian, interleaved; an hour or eight of programme as a decoder, a capture card or
 * a WAV file delivers it): `get` without a float copy of the stream -- half the memory the float call's caller holds, and no decode pass.
 * pcm_d = n_frames frames of n_channels int16 values (device pointer).
 * Definition: with f = what awm_pcm_decode_d (ctx, pcm_d, n_frames * n_channels, 16, 0, 0, f) writes -- float (v) * (1 / 32768), exact --
 * every call below returns, field for field and bit for bit, what its float twin (the same name without _s16) returns for f.
 * Paths: the kernels that read PCM on the long-stream path -- the dB kernels of the approximate search (K4), of the refinement (K4s) and
 * of the block decoder (K4b), and the silence scan of CLIP mode -- are instantiated for 16-bit input: a value is converted once, where
 * it leaves global memory, and nothing behind the load differs.  Chunks and lanes are views of pcm_d.  The ClipDecoder's two padded copies
 * (a block + 5 frames each) stay 16-bit, in the workspace the float call uses for them, and are read by the same kernels.  With default
 * parameters the call launches no decode of the stream or of a chunk, reserves no float PCM workspace and launches none of the float dB
 * kernels, for any stream length, chunk count and key count (scopes sync_db_s16_kernel(approx / refine / block), resample_s16_kernel).
 * Exceptions, both bounded by what one lane works on and both given back by awm_ctx_trim: while detect_speed, detect_speed_patient or
 * try_speed is set, a lane decodes the CHUNK it runs the speed part on into its grow-only float workspace (the speed search and the
 * stretch have no 16-bit form; the un-stretched decoders of that chunk still read the 16-bit values); and awm_get_watermark_rate_s16_d at
 * a rate that only the VResampler takes decodes the stream on its lane first.  At a rate the fixed-ratio resampler takes, the resampler
 * -- the form the float call launches -- reads the 16-bit values and writes the lane's 44.1 kHz float copy as in the float call; at 44100
 * the call is awm_get_watermark_s16_d.
 * Alignment: any even address.  A stereo stream whose frames are 4-byte aligned loads whole frames (8 bytes per lane where a lane's two
 * frames are 8-byte aligned); a stereo stream on an address that is only 2-byte aligned, and mono samples off a 4-byte boundary, take
 * 2-byte loads with the same bits.  Nothing outside the stream's values is read.
 * Refusals, AWM_ERR_ARG with nothing enqueued and the outputs untouched: an odd pcm_d; NULL with n_frames > 0; n_channels < 1; whatever
 * the float twin refuses; and any call while awm_debug_set_refine_form selects a form other than the default (4) -- only the default
 * forms of K4s have 16-bit instantiations.  n_frames == 0 behaves like the float twin.
 * Not offered: the file level and the command line, which convert their files' formats themselves (keeping a 16-bit WAV's bytes as the
 * resident stream is the obvious follow-up); awm_decode_chunk*_d, the sharded and awm_multi_* forms; other sample formats; the speed
 * search (K12, K15) on 16-bit input; the clip batches have forms of their own above, whose long clips keep their present path.  The `add`
 * side for whole streams and "watermark, then verify": awm_add_watermark_s16_d and awm_add_get_watermark_s16_d. */
int awm_get_watermark_s16_d (awm_ctx *ctx, const uint8_t key[16], const int16_t *pcm_d, size_t n_frames, int n_channels,
                             size_t max_out, awm_pattern *out);
int awm_get_watermark_keys_s16_d (awm_ctx *ctx, const uint8_t *keys, int n_keys, const int16_t *pcm_d, size_t n_frames, int n_channels,
                                  size_t max_out, awm_pattern *out, int *key_of_pattern);
int awm_get_watermark_rate_s16_d (awm_ctx *ctx, const uint8_t key[16], const int16_t *pcm_d, size_t n_frames, int n_channels,
                                  int sample_rate, size_t max_out, awm_pattern *out);
/* ... and the kernel level on such a stream: the twins of awm_sync_fft_d (K4), awm_sync_search_d (K4, K4s, the scans, the silence scan;
 * BLOCK and CLIP mode) and awm_block_soft_bits_d (K4b, K7).  Same definition, alignment, refusals and "not offered" as above. */
int awm_sync_fft_s16_d (awm_ctx *ctx, const int16_t *pcm_d, size_t n_frames, int n_channels, size_t index, size_t frame_count,
                        const char *want_frames, size_t first, size_t last, float *db_out_d, char *have_out_d);
int awm_sync_search_s16_d (awm_ctx *ctx, const uint8_t key[16], const int16_t *pcm_d, size_t n_frames, int n_channels, int clip_mode,
                           size_t max_out, uint64_t *index, double *quality, int *block_type);
int awm_block_soft_bits_s16_d (awm_ctx *ctx, const uint8_t key[16], const int16_t *pcm_d, size_t n_frames, int n_channels,
                               const uint64_t *index, size_t n_blocks, float *out, int *ok);
/* decode() of one chunk only (wmget.cc:886-939) -- the unit `get` is sharded by */
int awm_decode_chunk_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames,
                        int n_channels, int first_chunk, size_t max_out, awm_pattern *out);

/* decode() for several chunks that live in one resident buffer (chunk i = frames [first_frame[i], first_frame[i] +
 * chunk_frames[i]) of pcm_d); device work is batched across the chunks, every chunk is searched / combined on its own
 * exactly like awm_decode_chunk_d.  first_is_stream_start != 0 runs the ClipDecoder on chunk 0.  Pattern times are
 * relative to their chunk; chunk_of_pattern[j] tells which chunk pattern j belongs to (patterns are ordered by chunk,
 * then time).  This is the per-rank unit of a sharded `get`. */
int awm_decode_chunks_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels,
                         int n_chunks, const uint64_t *first_frame, const uint64_t *chunk_frames, int first_is_stream_start,
                         size_t max_out, awm_pattern *out, int *chunk_of_pattern);

/* File level = the reference's own entry points add_watermark (key, infile, outfile, bits) and get_watermark (key_list,
 * infile, orig_pattern) (wmcommon.hh:226-228, wmadd.cc:620-657, wmget.cc:971-1013) with a GPU context.  The file is streamed
 * through page-locked staging buffers in its own sample format (bounded host memory: tile loop for `add` at 44.1 kHz, chunked
 * staging otherwise) and converted on the device.  raw_* = NULL: WAV (RIFF / RF64) by header, like --input-format auto;
 * else headerless PCM as with --format raw --raw-rate/--raw-channels/--raw-bits/--raw-encoding/--raw-endian.
 * awm_get_watermark_file returns the number of patterns found (at most max_out are written), < 0 on error. */
typedef struct { int n_channels, sample_rate, bit_depth, encoding /* 0 signed, 1 unsigned, 2 float */, big_endian; } awm_raw_format;
int awm_add_watermark_file (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const char *in_path, const char *out_path,
                            const awm_raw_format *raw_in, const awm_raw_format *raw_out);
/* add_stream_watermark (key, in_stream, out_stream, bits, zero_frames) (wmcommon.hh:226, wmadd.cc:448-618) on files: the input is the
 * continuation of a stream that is `zero_frames` samples in (hls.cc:279 watermarks a segment this way); zero_frames = 0 is
 * awm_add_watermark_file.  At 44.1 kHz the start offset costs nothing (a frame counter and a limiter block phase); at other rates (those
 * awm_add_watermark_segments_rate_d takes) the output is computed from a window of 44.1 kHz frames around the input, at its global
 * indices (the resamplers' skip leaves them in the state zeros would have, resample.cc:150-168): no zero is stored, the cost does not
 * depend on zero_frames.  While an SNR meter is running (`--snr`, or awm_ctx_snr_begin by the caller) the zeros are still materialised in HBM,
 * as before: the powers are those of the whole zero-prefixed stream. */
int awm_add_stream_watermark_file (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const char *in_path, const char *out_path,
                                   const awm_raw_format *raw_in, const awm_raw_format *raw_out, size_t zero_frames);
/* awm_add_watermark_file / awm_add_stream_watermark_file of ONE input file with n_payloads payloads and one key: out_path[p] is byte for
 * byte the file awm_add_stream_watermark_file (ctx, key, payload_hex[p], in_path, out_path[p], raw_in, raw_out, zero_frames) writes.  At
 * 44.1 kHz the input is read, uploaded and sample-decoded once and pushed through an awm_add_stream with n_payloads payloads; every
 * payload has an output stage of its own (a ring of page-locked tiles, a writer), so the files are written side by side.  Host memory
 * stays bounded whatever the file length and n_payloads: the tile is the largest number of 1024-sample frames, at most 4096 and never
 * below 128, for which the output rings together -- n_payloads rings x 4 slots x tile x bytes per output frame -- stay within 1 GiB of
 * page-locked memory (stereo 16 bit: 4096 frames up to 16 payloads, 1024 frames at 64).  The additional rings belong to the call.
 * At another sample rate (those awm_add_watermark_segments_rate_d takes) the input is read, uploaded and sample-decoded ONCE into HBM and
 * the outputs are produced there in passes of at most four payloads -- zero_frames == 0: awm_add_watermark_payloads_d, else
 * awm_add_watermark_segments_rate_d with the pass's payloads as segments that alias the input -- and written one after the other, in payload
 * order, from output buffers that the passes reuse.
 * `snr` in the parameters, n_payloads == 1, more than AWM_ADD_STREAM_MAX_PAYLOADS payloads and rates without fixed-ratio tables: a loop
 * over awm_add_stream_watermark_file.  n_payloads == 0: returns 0 and touches nothing.
 * AWM_ERR_ARG before any file is opened or truncated: a NULL pointer, a payload that does not parse, two equal output paths, an output
 * path equal to the input path.  Information lines appear once per output, in payload order. */
int awm_add_watermark_payloads_file (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads,
                                     const char *in_path, const char *const *out_path,
                                     const awm_raw_format *raw_in, const awm_raw_format *raw_out);
int awm_add_stream_watermark_payloads_file (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads,
                                            const char *in_path, const char *const *out_path,
                                            const awm_raw_format *raw_in, const awm_raw_format *raw_out, size_t zero_frames);
int awm_get_watermark_file (awm_ctx *ctx, const uint8_t key[16], const char *in_path, const awm_raw_format *raw_in,
                            size_t max_out, awm_pattern *out);
/* add_watermark (key, infile, outfile, bits) followed by get_watermark (key, outfile) ("watermark, then verify that the payload decodes":
 * wmadd.cc:620-657 + wmget.cc:971-1013; the file twin of awm_add_get_watermark_d): the input is read once and the output is never read
 * back -- the output stage decodes the bytes it has just encoded for the file (the samples as the file holds them, after its sample format's
 * quantisation) into HBM and `get` runs there.  Same file and same pattern list as the two calls; returns the number of patterns. */
int awm_add_get_watermark_file (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const char *in_path, const char *out_path,
                                const awm_raw_format *raw_in, const awm_raw_format *raw_out, size_t max_out, awm_pattern *out);
int awm_get_watermark_keys_file (awm_ctx *ctx, const uint8_t *keys, int n_keys, const char *in_path, const awm_raw_format *raw_in,
                                 size_t max_out, awm_pattern *out, int *key_of_pattern);

/* chunk plan of WavChunkLoader (wavchunkloader.cc:54-163) for a stream of n_frames samples per channel:
 * chunk i covers [first_frame[i], first_frame[i] + chunk_frames[i]) and reports times offset by
 * time_offset[i] seconds.  Pure host.  Returns the chunk count (<= max_out filled).  The chunks are the
 * unit `get` is sharded by across GPUs. */
int awm_plan_chunks (size_t n_frames, size_t max_out, uint64_t *first_frame, uint64_t *chunk_frames, double *time_offset);
/* ResultSet::merge + sort (wmget.cc:215-316) over per-chunk pattern lists that were decoded elsewhere
 * (other ranks): `patterns` holds the chunks' patterns back to back in chunk order with times already
 * offset, chunk_count[i] patterns for chunk i.  Result written to out (<= max_out), count returned. */
int awm_merge_patterns (const uint8_t key[16], const awm_pattern *patterns, const int *chunk_count, int n_chunks,
                        size_t max_out, awm_pattern *out);

/* ---- one stream over several GPUs -------------------------------------------------------------------------------------------
 * The stream is the concatenation of the ranks' spans (rank order; every span but the last non-empty one a whole number of
 * 1024-sample frames), one context per GPU.  What the algorithm couples across a span boundary is all that travels:
 *   add   one frame each way (3-frame overlap-add, wmadd.cc:228-238) and the limiter's per-second maxima of the seconds that
 *         straddle span edges (limiter.cc:90-124): one exchange of edge frames + one max-reduction.
 *   get   The reference's chunks (wavchunkloader.cc:75-84) stay the semantic unit -- local mean, n_best and the A / B
 *         combination are per chunk -- but the WORK of a chunk is split by position: a rank computes the sync scores
 *         (syncfinder.cc:171-256), refines (:393-458) and extracts the soft bits (wmget.cc:67-108) of the candidate starts that lie in its
 *         span, for which it needs one block + 2 frames of its successor's samples (the "overlap stitch", 18 MB for stereo);
 *         the ranks that share a chunk exchange its raw scores (32 B per frame of audio: the "score gather"), select the
 *         candidates redundantly (deterministic), exchange the few refined scores and the blocks' soft bits (3.4 KB per block),
 *         and share the Viterbi decodes.  Rank 0 merges the patterns (wmget.cc:288-316).  Work per rank is proportional to its
 *         span (balanced to within a block), results are identical to awm_get_watermark_d on the whole stream.
 * The transport is the caller's: three callbacks (RCCL / torch.distributed in audiowmark_amd/sharded.py, hipMemcpyPeer between the
 * threads of one process in awm_multi_*).  Every rank calls the entry point with the same span list; all sizes are known on both
 * sides of every transfer.  Each callback returns 0 or an error (the entry point then fails with AWM_ERR_GENERIC). */
typedef struct awm_comm
{
  void *user;
  int   rank, world;
  /* point-to-point round: all transfers posted together, complete on return.  *_d: device memory (the data is ready on the
   * context's stream when the callback is entered, and the callback's writes are visible to that stream when it returns);
   * *_h: host memory (small control data). */
  int (*exchange_d) (void *user, int n_send, const void *const *send, const size_t *send_bytes, const int *send_to,
                     int n_recv, void *const *recv, const size_t *recv_bytes, const int *recv_from);
  int (*exchange_h) (void *user, int n_send, const void *const *send, const size_t *send_bytes, const int *send_to,
                     int n_recv, void *const *recv, const size_t *recv_bytes, const int *recv_from);
  /* element-wise maximum over all ranks of n unsigned 32 bit words in device memory, in place (the limiter maxima: non-negative
   * floats order like their bit patterns) */
  int (*all_reduce_max_u32_d) (void *user, uint32_t *data, size_t n);
} awm_comm;
/* add_watermark core for this rank's span (out_d: span_frames[rank] * C floats); 44.1 kHz streams only */
int awm_sharded_add_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const float *pcm_in_d, float *out_d, int n_channels,
                       const uint64_t *span_frames /* [world] */, const awm_comm *comm);
/* get_watermark core; the merged pattern list arrives on rank 0 (return value = its length, at most max_out written), the other
 * ranks return 0 */
int awm_sharded_get_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, int n_channels, const uint64_t *span_frames /* [world] */,
                       const awm_comm *comm, size_t max_out, awm_pattern *out);
/* the plan behind awm_sharded_get_d, for tests and balance checks (pure host): for every (chunk, rank) the range of candidate start
 * frames [first_sf, first_sf + n_sf) of the chunk that rank works on.  Returns the number of entries (chunks * world). */
int awm_sharded_plan (const uint64_t *span_frames, int world, size_t max_out, int *chunk, int *rank, uint64_t *first_sf, uint64_t *n_sf);

/* The same on the GPUs of ONE process (the command line's --gpus / AWM_DEVICES): one context per device, one host thread per
 * context inside the call, hipMemcpyPeer as transport.  span i lives on ctxs[i]'s device at pcm_d[i] (several contexts may share
 * a device). */
int awm_multi_add_d (awm_ctx *const *ctxs, int n_ctx, const uint8_t key[16], const char *payload_hex, const float *const *pcm_in_d,
                     float *const *out_d, int n_channels, const uint64_t *span_frames);
int awm_multi_get_d (awm_ctx *const *ctxs, int n_ctx, const uint8_t key[16], const float *const *pcm_d, int n_channels,
                     const uint64_t *span_frames, size_t max_out, awm_pattern *out);

/* Batches of independent clips over the contexts of one process (BASELINE configs[4] on several GPUs): clip i lives on the device of
 * ctxs[ctx_of_clip[i]] and is handled there -- one host thread per context runs awm_add_watermark_batch_keys_d /
 * awm_get_watermark_batch_keys_d on its share, results come back in clip order.  Replicas: nothing travels between the devices
 * (reference: n_clips independent `audiowmark add` / `get` runs, wmadd.cc:620-657, wmget.cc:764-884).  keys = n_clips * 16 bytes, or
 * NULL with one_key != NULL: that key for every clip.  The settings in force for every context are the calling thread's / ctxs[0]'s. */
int awm_multi_add_watermark_batch_d (awm_ctx *const *ctxs, int n_ctx, const int *ctx_of_clip, const uint8_t *keys, const uint8_t *one_key,
                                     const char *payload_hex, size_t n_clips, const float *const *pcm_in_d, float *const *out_d,
                                     const size_t *n_frames, int n_channels);
int awm_multi_get_watermark_batch_d (awm_ctx *const *ctxs, int n_ctx, const int *ctx_of_clip, const uint8_t *keys, const uint8_t *one_key,
                                     size_t n_clips, const float *const *pcm_d, const size_t *n_frames, int n_channels,
                                     size_t max_out_per_clip, awm_pattern *out, int *n_out);

/* Helpers of a context: contexts on other GPUs that the file level `get` (awm_get_watermark_file / _keys_file, the command line) may
 * spread a long single-key stream over (awm_multi_get_d after the stream has been read through `ctx`; its spans travel device to
 * device).  The helpers stay the caller's; n_helpers = 0 takes them away.  The command line fills them from AWM_DEVICES=0,1,... */
int awm_ctx_set_helpers (awm_ctx *ctx, awm_ctx *const *helpers, int n_helpers);

/* ---- speed detection (reference wmspeed.cc:622-781) ------------------------------------
 * `get --detect-speed`: the reference looks for the replay speed (0.8 .. 1.25) of the watermark before decoding, by
 * correlating the sync pattern with a half-rate STFT of a 25 / 50 s clip over a grid of speeds, and decodes the stream a
 * second time stretched back to speed 1 (wmget.cc:886-927).  awm_set_speed_params switches that part of decode() on for
 * awm_get_watermark_d / awm_decode_chunk(s)_d (Params::detect_speed, detect_speed_patient, try_speed, test_speed;
 * wmcommon.hh:49-52); patterns found on the stretched stream carry the speed in awm_pattern.speed.
 * The stretch is zita-resampler's VResampler (resample.cc:96-125), restated like the fixed-ratio Resampler: bit parity
 * with the library is unpinned.  On the device the resampler's phase comes from the exact product instead of zita's
 * accumulated double (differs by its accumulated rounding only): stretched PCM is bit-exact against the exact-phase restatement
 * (tests/_speed.py var_resample32 on awm_var_resample_table) and agrees to ~1e-7 with zita's accumulated phase. */
void awm_set_speed_params (int detect_speed, int detect_speed_patient, double try_speed, double test_speed);
/* resample_ratio_truncate (resample.cc:96-119): frames the call produces / the call itself (out_d: n_out_frames frames) */
size_t awm_resample_ratio_frames (size_t n_frames, int n_channels, int rate, double ratio, double max_in_seconds);
int awm_resample_ratio_d (awm_ctx *ctx, const float *pcm_in_d, size_t n_frames, int n_channels, int rate, double ratio,
                          double max_in_seconds, float *out_d, size_t n_out_frames);
/* detect_speed for one key (wmspeed.cc:622-781) on resident PCM: returns 1 if decoding at *speed_out should be tried
 * (quality > 0.4 and speed outside 0.9999 .. 1.0001), 0 if not, < 0 on errors; speed / quality are filled in either way */
int awm_detect_speed_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int rate,
                        int patient, double *speed_out, double *quality_out);
/* the pieces, for parity tests: get_best_clip_location (wmspeed.cc:555-577); SpeedSync::prepare_mags for one centre speed
 * (:204-268; out is host memory, [row][510 sync frames sorted by frame][umag, dmag], returns the row count); one
 * run_search pass (:461-492, 683-719; scores sorted by speed, returns their number) */
int awm_speed_clip_location_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int rate,
                               double seconds, int candidates, double *location);
int awm_speed_mags_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int rate,
                      double clip_location, double center, double seconds, size_t max_rows, float *out);
int awm_speed_scan_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int rate,
                      double clip_location, double seconds, double step, int n_steps, int n_center_steps,
                      const double *speeds, int n_speeds, size_t max_out, double *out_speed, double *out_quality);

/* detect_speed for a batch of clips, the batch of awm_detect_speed_d: clip i with keys (16 bytes) or keys + 16 i (key_per_clip != 0).
 * The passes of the search run in lockstep for sub-groups of clips -- one launch per kernel and pass, one synchronisation between
 * passes for the whole sub-group (the batch forms of K12 - K15, speed.hip) -- and every clip's result is bit for bit that of the
 * one-clip call: use_out[i] = 1 / 0 as awm_detect_speed_d returns them, speed_out[i] / quality_out[i] its speed and quality; a clip
 * under 0.25 s has 0, 0, 0.  A clip on which the one-clip call fails (digital silence: AWM_ERR_ARG, "failed to setup vresampler")
 * has that error code in use_out[i] and 0, 0; the other clips are not affected and the call returns 0.  The clips are read where
 * they lie and need 4 byte alignment only.  AWM_ERR_ARG with nothing enqueued and the outputs untouched: a null pcm_d[i] with
 * n_frames[i] > 0, n_channels < 1, rate <= 0.  n_clips == 0 returns 0.
 * A sub-group is as many clips, in order, as fit a byte budget for the first pass's scratch (sub + mags, about 1.25 GB per 30 s
 * stereo clip); awm_debug_set_speed_batch_bytes changes it (0: the default), awm_speed_batch_plan (pure host) returns the number of
 * sub-groups and writes every clip's sub-group (-1: under 0.25 s) and every sub-group's bytes (n_clips entries at most; may be null);
 * budget_bytes 0: the current setting.  Memory: the default budget is 32 GiB, the largest of three measured values (4 / 12 / 32 GiB;
 * larger ones were not measured, the times were still falling).  The scratch is per lane and grow-only: one call with 27 or more
 * stereo clips of 30 s grows the lane's scratch to about 32 GiB, and it stays until awm_ctx_trim; a caller short of memory sets a
 * smaller budget first (a sub-group of one clip asks for 1.25 GB).  awm_debug_speed_batch_launches: launches of the batch kernels so far (K15: gather + energy). */
int  awm_detect_speed_batch_d (awm_ctx *ctx, const uint8_t *keys, int key_per_clip, size_t n_clips, const float *const *pcm_d,
                               const size_t *n_frames, int n_channels, int rate, int patient, double *speed_out, double *quality_out,
                               int *use_out);
void awm_debug_set_speed_batch_bytes (size_t bytes);
size_t awm_debug_speed_batch_bytes (void);             /* the budget in force */
int  awm_speed_batch_plan (size_t n_clips, const size_t *n_frames, int n_channels, int rate, int patient, size_t budget_bytes,
                           int *group_of_clip, size_t *bytes_of_group);
void awm_debug_speed_batch_launches (int *k12, int *k13, int *k14, int *k15);
/* (A / B) how the batches of clips (awm_get_watermark_batch_d and its forms) work under a speed parameter.  0, the default: every clip
 * over the work lanes in parallel with the one-clip search.  1: the short clips keep their groups (float or 16-bit, 44.1 kHz or another
 * fixed-ratio rate); after stage 0 of a group the speed search of its clips runs as a batch on the slices (awm_detect_speed_batch_d's
 * way, on the group's lane, whose search scratch grows to the byte budget), the stretched decodes of the clips with a speed run over the
 * lanes afterwards; measured slower than 0 (profiles/get_batch_speed).  2: one clip after the other on the context's own lane (what the batches did before; kept for
 * tools/gpu_get_batch_speed.py).  The results are the same in all three. */
void awm_debug_set_speed_batch (int mode);
/* the batch of awm_speed_scan_d: ONE pass over several clips in one launch per kernel, clip i with its own clip location and its
 * own n_speeds[i] speeds (`speeds`: all lists back to back); scores of clip i sorted by speed at out_*[i * max_out_per_clip ...],
 * n_out[i] their number (or the clip's error code) */
int  awm_debug_speed_scan_batch_d (awm_ctx *ctx, const uint8_t *keys, int key_per_clip, size_t n_clips, const float *const *pcm_d,
                                   const size_t *n_frames, int n_channels, int rate, const double *clip_locations, double seconds,
                                   double step, int n_steps, int n_center_steps, const double *speeds, const int *n_speeds,
                                   size_t max_out_per_clip, double *out_speed, double *out_quality, int *n_out);

/* host side pieces of the search (pure host, no GPU): select_n_best_scores (wmspeed.cc:494-531; in place, returns the new
 * count), score_smooth_find_best (:397-428), and the two halves of get_clip_locations (:533-553): the sample positions that
 * are hashed, and the candidate locations drawn from the generator re-seeded with the SHA-1 of those samples
 * (Random::seed_from_hash, random.cc:184-190) */
int    awm_speed_select_n_best (double *speed, double *quality, int count, int n);
double awm_speed_smooth_best (const double *speed, const double *quality, int count, double step, double distance);
size_t awm_speed_clip_positions (const uint8_t key[16], size_t n_values, size_t max_out, uint64_t *positions);
int    awm_speed_clip_candidates (const uint8_t key[16], const float *hashed_values, size_t n, int candidates, double *locations);
/* the coefficient table awm_resample_ratio_d uses for `ratio` (VResampler::setup (ratio, nchan, 16): 257 phases x hl taps, dense, row
 * major, before the padding of the device copy): returns its size 257 * *hl in floats and copies min (size, max_floats) of them to out
 * (out may be null); < 0 if the ratio is refused (ratio < 1 / 16 or > 256) */
int    awm_var_resample_table (double ratio, float *out, size_t max_floats, int *hl);

/* A / B hooks for measurements (tools/gpu_variants.py): the previous formulation of two kernels stays selectable so that a change can be
 * timed against it in one process, on the same data, with the same clocks.  Results are bit-identical either way (tests).
 *   viterbi_super: 1 (default) three trellis rounds per launch with the metrics exchanged through LDS / 0 one round per launch
 *                  (tests/test_gpu_viterbi_edges.py runs every input of its fixture in both forms)
 *   sliding3:      1 (default) refinement with three bins of one channel per lane / 0 two bins of both channels (stereo) */
void awm_debug_set_viterbi_super (int on);
void awm_debug_set_viterbi_persistent (int on); /* K8: 1 ONE launch per batch of decodes (8 resident workgroups per decode meeting at a counter in global
                                                 * memory every 12 trellis steps) | 0 the chain of 14 dependent launches | -1 (default) chosen per process from
                                                 * the measured cost of a dependent launch on this host (awm_ctx_create probes it): the chain where launches
                                                 * are cheap, the one-launch kernel where they are not.  Bits and error values are identical. */
double awm_debug_dependent_launch_us (void);    /* the probe's result (microseconds per empty dependent launch; -1 before the first context) */
int  awm_debug_viterbi_one_launch_in_use (void);
void awm_debug_set_sliding3 (int on);          /* (rounds 3 - 5: refine form 3 / 0) */
/* K4s, the refinement's sliding DFT for stereo streams (reference SyncFinder::search_refine -> sync_fft, syncfinder.cc:393-458, 560-605):
 *   0  two bins of both channels per lane | 3  three bins of one channel per lane (rounds 3 - 5) | 4 (default) the same arithmetic in a
 *   straight-line step with the wave-uniform rules on the scalar unit: outputs of 0, 3, 4 are identical to the last bit |
 *   5  the update term of the recurrence accumulated in float (state, rotation and Hann combination stay double): the level of a float
 *      FFT, which is what the reference's FFTW is; NOT bit-identical to 4 -- gated by the census in DESIGN.md section 4 */
void awm_debug_set_refine_form (int form);
int  awm_debug_refine_form (void);
void awm_debug_set_k4s_ablate (int flags);     /* measurement only (tools/gpu_k4s_alone.py): 8 = awm_debug_sync_db_sliding_d runs forms 4 / 5 without their stores */
/* K4s alone on resident PCM (stereo or mono): stream i = `count` (<= 65) windows of 1024 samples starting at base_d[i] + 8 o; writes
 * out_d[i][band 0..80][ld] (dB summed over the channels) in the form in force.  For the tests that pin forms 0 / 3 / 4 against each other.
 * ld = 64 (measurement): the refinement's gathered layout with a synthetic table instead (bands 0..59 are the rows): out_d[i][60][64], and with
 * forms 4 / 5 the 65th values at out_d + n_streams * 60 * 64 (n_streams * 60 floats more). */
int  awm_debug_sync_db_sliding_d (awm_ctx *ctx, const float *pcm_d, size_t n_frames, int n_channels, const long long *base_d, size_t n_streams,
                                  int count, int ld, float *out_d);
/* K4s alone as the refinement launches it (tests only): the gathered layout with every table from the caller, all of them device pointers.
 * Stream s = plane * rows_per_plane + w has count_d[s] (0 .. count0 <= 65) windows from base_d[s] + 8 o and writes band b of offset o to
 *   out_d[(slot * 60 + band_pos_d[(slice * rows_per_plane + w) * 81 + b]) * ld + o]   (255: the band is dropped),
 *   slot = plane * rows_per_plane + row_perm_d[slice * rows_per_plane + w],  have_d[slot * have_stream_stride + o] = the offset was transformed,
 * and with tail_d (forms 4 / 5, stereo) offset 64 to tail_d[slot * tail_stream_stride + row] instead, so that ld may be 64.
 * [first, last) is the non-silent value range of the skip rules; stream_range_d (optional, [slices][2]) replaces it per stream by the range
 * of slice range_index_d[s / range_div] (s / range_div without range_index_d; first < 0: nothing but silence), and with tables_per_slice = 1
 * row_perm_d / band_pos_d hold one table per slice (slice = 0 otherwise).  Counts and windows are checked on the host (one synchronisation). */
int  awm_debug_sync_db_sliding_rows_d (awm_ctx *ctx, const float *pcm_d, size_t n_frames, int n_channels, const long long *base_d, const int *count_d,
                                       size_t n_streams, int count0, int rows_per_plane, const int *row_perm_d, const unsigned char *band_pos_d,
                                       long long first, long long last, const long long *stream_range_d, const int *range_index_d, int range_div,
                                       int tables_per_slice, int ld, float *out_d, float *tail_d, long long tail_stream_stride, char *have_d,
                                       long long have_stream_stride);
/* ... on a stream of SIGNED 16-BIT PCM (awm_get_watermark_s16_d above): K4s in the product's gathered layout, instantiated for 16-bit
 * input.  Definition: every cell, have flag and untouched cell is bit for bit what awm_debug_sync_db_sliding_rows_d writes for the decoded
 * stream.  Paths: stereo the default form (4, rows of 64 + tail), mono sync_db_sliding_kernel<1>; the wave-uniform base and one 32-bit
 * lane offset of the float kernel are kept.  Alignment: any even address; stereo frames that are 4-byte aligned are loaded whole, a base
 * that is only 2-byte aligned takes 2-byte loads.  Refusals: those of the float call, an odd pcm_d, and a form other than the default
 * (awm_debug_set_refine_form): AWM_ERR_ARG, nothing enqueued.  Not offered: the other forms, awm_debug_sync_db_sliding_d's bands layout. */
int  awm_debug_sync_db_sliding_rows_s16_d (awm_ctx *ctx, const int16_t *pcm_d, size_t n_frames, int n_channels, const long long *base_d,
                                           const int *count_d, size_t n_streams, int count0, int rows_per_plane, const int *row_perm_d,
                                           const unsigned char *band_pos_d, long long first, long long last, const long long *stream_range_d,
                                           const int *range_index_d, int range_div, int tables_per_slice, int ld, float *out_d, float *tail_d,
                                           long long tail_stream_stride, char *have_d, long long have_stream_stride);
void awm_debug_set_soft_bits_generic (int on); /* K7: one thread per soft bit for every shape (the fallback kernel) | four bits per wave */
/* The block decoder's dB pass (K4b) and soft bits (K7) as awm_block_soft_bits_d launches them, with the dB planes made visible (tests only).
 * The dB workspace is filled with the 32-bit pattern `fill` before K4b runs; the planes of the accepted blocks go to
 * planes_out_d[slot][channel][band 0..80][ld] (device, planes_values floats, ld = awm_debug_block_plane_ld()), their soft bits to
 * soft_out[slot][858] (host), slot_out[i] = the slot of block i or -1 (the block runs past the samples, as ok[i] = 0 of awm_block_soft_bits_d).
 * slice_range_d (optional, device, [n_slices][2]) with slice_frames is the mode of a row of padded clips: block i belongs to slice
 * index[i] / slice_frames, whose values that are not digital silence are [first, last) as absolute value indices (first < 0: none); frames
 * outside get -96 dB without a transform, tiles K7 does not read are not written (where K7 is the one-thread-per-bit kernel, which loads
 * every cell, all are), and K7 gets the same ranges.
 * Arguments are checked on the host before anything is launched (at most one synchronisation): AWM_ERR_ARG for up to 3 channels, 1 .. 64
 * blocks, a planes buffer too small for n_blocks blocks, slices that do not fit the samples, blocks behind the last slice, ranges outside
 * 0 <= first <= last <= n_frames * n_channels. */
int  awm_debug_block_plane_ld (awm_ctx *ctx);
int  awm_debug_block_db_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, const uint64_t *index,
                           size_t n_blocks, uint32_t fill, const long long *slice_range_d, size_t n_slices, size_t slice_frames,
                           float *planes_out_d, size_t planes_values, float *soft_out, int *slot_out);
/* K7 alone on dB planes of the caller, planes_d[block][channel][81][ld] (device, planes_values floats): soft_out[block][858] (host).
 * block_base_d [n_blocks], slice_range_d [n_slices][2] and range_index_d [n_blocks] (device, all three or none) are the padded-clip mode:
 * block b starts at sample block_base_d[b] of a buffer whose slice range_index_d[b] has the range slice_range_d[..]; checked on the host
 * like the arguments above (bases and ranges within 0 .. 2^40). */
int  awm_debug_soft_bits_planes_d (awm_ctx *ctx, const uint8_t key[16], const float *planes_d, size_t planes_values, size_t n_blocks, int n_channels,
                                   const long long *block_base_d, const long long *slice_range_d, const int *range_index_d, size_t n_slices,
                                   float *soft_out);
void awm_debug_set_scan_generic (int on);      /* K5w: 1 the approximate search takes launch_sync_scan_window's fallback, the generic K5 (scores identical) | 0 (default) the streaming kernel */
int  awm_debug_scan_generic_launches (void);   /* K5w: how often launch_sync_scan_window has taken that fallback in this process, by the switch or by its own conditions */
void awm_debug_set_chunk_stagger (int mode); /* get: phase offset between the chunk lanes -- 0 all chunks start together | 1 chunk i + 1 behind chunk i's
                                             * dB kernel | 2 behind its scan | -1 (default) 1 for streams of up to `lanes` chunks, 2 for longer ones */
void awm_debug_set_resample_phase (int on);  /* K10: 1 (default) the phase-per-thread kernel for stereo 48 <-> 44.1 kHz | 0 the generic kernel (outputs identical) */
/* K10s alone: outputs out0 .. out0 + n_out - 1 of the fixed-ratio resampler rate_in -> rate_out to out_d[0 ..], from the frames in0 .. in0 +
 * n_in - 1 of the stream at in_d (everything else reads as zero): the same values awm_resample_d writes for those outputs of the whole
 * stream.  *phase_form_used: 1 if the phase-per-thread kernel ran (stereo 48 <-> 44.1 kHz, 8-byte aligned pointers, out0 a multiple of np,
 * the switch above on), 0 for K10w. */
int  awm_debug_resample_span_d (awm_ctx *ctx, const float *in_d, size_t n_in, uint64_t in0, uint64_t out0, size_t n_out, int n_channels,
                                int rate_in, int rate_out, float *out_d, int *phase_form_used);
void awm_debug_set_get_overlap (int on);    /* file level get: 1 (default) the chunks start while the rest of the stream is still crossing PCIe (a loader thread, a mark per
                                             * tile; streams of announced length at 44.1 kHz with two chunks or more) | 0 the whole stream first (rounds 1 - 5) */
void awm_debug_set_speed_compare_wide (int on); /* K14: 1 all relative speeds of a centre (<= 12) in one thread / 0 (default) groups of six: measured slower, see hip/speed.hip */
void awm_debug_set_speed_compare_fold (int on); /* K14: 1 (default) the groups of six of a (state range, centre) are neighbouring workgroups on one XCD / 0 a grid dimension of their own */
void awm_debug_set_resample_var_mode (int mode); /* K12: bit 0 the stereo input window of a tile through LDS | bit 1 a workgroup keeps its coefficient
                                             * table for several tiles (default 2; outputs identical) */
void awm_debug_set_speed_overlap (int on);   /* get with a speed search: 1 (default) the plain decode of the chunks runs beside the speed part, on lanes
                                             * of its own | 0 after it (the reference's order of work; the pattern lists are the same) */
int  awm_debug_frame_mod_tables_d (awm_ctx *ctx, const uint8_t *keys, size_t n_keys, const char *payload_hex, int8_t *tables_out);
                                             /* the frame_mod tables as K16 builds them (wmadd.cc:86-162), n_keys x 2 x 2226 x 81 bytes to host memory:
                                              * for the test that they equal awm_tab_frame_mod key by key */
int  awm_debug_clip_key_tables_check_d (awm_ctx *ctx, const uint8_t *keys, size_t n_keys, long long mismatch_out[9]);
                                             /* the tables `get` needs per key of a clip batch (K16g: sync chains, row frames, want list, gathered layout,
                                              * mix entries, bit order) built on the device, group by group, against the host's build of the same tables:
                                              * mismatch_out[i] = differing elements per table (all 0 = identical) */
void awm_debug_set_key_tables_on_device (int on);   /* batches with one key per clip: 0 the tables from host threads | `add`'s frame_mod tables (K16) and `get`'s sync / mix / bit order tables (K16g) built on the device: 1 (default) `get` builds a group's tables one group ahead of its lane, 2 the tables of all (up to 4096) keys first (measured: the same time) */
void awm_debug_set_merge_decodes (int on);  /* get of a stream of 2 - 4 chunks: the chunks' Viterbi jobs as ONE batch at the end | per chunk (default: the step is faster) */
void awm_debug_set_add_batched (int on);   /* add of a batch of stereo clips: 2 (default) ONE launch per stage for many clips (block maxima, K2, limiter table, limiter: blockIdx.y =
                                            * the clip, spans sized for the batch), with a key per clip after the tables of all (up to 4096) keys | 1 the same with a
                                            * group's tables built while the previous group of 256 clips is watermarked | 0 four launches per clip on eight lanes; the
                                            * outputs are the same */
void awm_debug_set_add_slab_mb (int mb);   /* add: 0 (default) one fused add over the stream, then the limiter | > 0: in slabs of that many MB (cache experiment) */
void awm_debug_set_add_payloads_fused (int on);   /* awm_add_watermark_payloads_d, awm_add_mix_payloads_d: 1 (default) the fused kernel | 0 a loop over the single-payload path */
int  awm_debug_add_payloads_fused_in_use (void);  /* 1 if the last awm_add_watermark_payloads_d / awm_add_mix_payloads_d (also inside a stream push) ran the 44.1 kHz kernel (0 at every other rate) */
void awm_debug_set_add_payloads_rate_fused (int mode);  /* awm_add_watermark_payloads_d at another sample rate: 2 (default) shared down-resample + K2m + K10m where K10m applies | 1 shared
                                                         * down-resample + K2m, then K10 and K11 per output | 0 a loop over the single-payload path (as awm_debug_set_add_payloads_fused (0) at every rate) */
int  awm_debug_add_payloads_rate_fused_in_use (void);   /* which of these the last awm_add_watermark_payloads_d took: 2 | 1 (also: not stereo, another fixed ratio than 44.1 -> 48 kHz, a pointer
                                                         * that is only 4-byte aligned) | 0 (also: 44.1 kHz, one payload, a VResampler rate, workspaces that could not be reserved) */
int  awm_debug_add_s16_fused_in_use (void);       /* 1 if the last awm_add_watermark_s16_d / awm_add_get_watermark_s16_d ran without a decode and an encode of the stream, 0 if it went through the definition */
int  awm_debug_add_segments_fused_in_use (void);  /* 1 if the last awm_add_watermark_segments_d / _rate_d / _keys_d / _keys_rate_d took the fused path (one launch per stage), 0: segment by segment */
int  awm_debug_payload_tables_d (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads, int8_t *tables_out);
/* K16t alone: the templates of n_keys keys (16 bytes each) built on the device, 256 keys per launch, copied to out: n_keys x 360624 int16
 * (awm_tab_frame_mod_template's 2 x 2226 x 81 entries and the zeros up to a multiple of 16); out may be NULL (the launches alone).
 * K16t + K16p: the tables of n <= 1024 (key, payload) pairs, pair i with keys + 16 i, n x 2 x 2226 x 81 bytes == awm_tab_frame_mod per pair.
 * Both return AWM_ERR_ARG for a geometry K16t does not build (mix off, frames_per_bit != 2, a payload size other than 128 bits); the
 * fused path of awm_add_watermark_segments_keys_d takes the host's templates there. */
int  awm_debug_key_templates_d (awm_ctx *ctx, const uint8_t *keys, size_t n_keys, int16_t *out);
int  awm_debug_key_payload_tables_d (awm_ctx *ctx, const uint8_t *keys, const char *const *payload_hex, size_t n, int8_t *tables_out);
                                             /* K16p alone: the frame_mod tables of 1 .. 1024 payloads with one key, expanded on the device from the key's template,
                                              * n_payloads x 2 x block frames x 81 bytes to host memory (they equal awm_tab_frame_mod payload by payload);
                                              * tables_out NULL: the launch alone, on the context's stream (timing) */
void awm_debug_set_payloads_file_tile (int frames1024);   /* awm_add_watermark_payloads_file: tile of the fused path in 1024-sample frames (>= 128) | 0 (default) automatic */
int  awm_debug_add_payloads_tile (void);          /* outputs per pass of the fused kernel over the input (ADD_MULTI_TILE) */
void awm_debug_set_fft_pair (int on);      /* stereo add: both channels' transforms pipelined in one wave (default) | one after the other */
void awm_debug_set_clip_poison (int on);    /* clip batches: the padded slices are filled with NaNs before the copies are written (the copy writes a clip and 2048
                                            * frames of zeros on either side, not the rest of the padding: a consumer that read further would change its result) */
size_t awm_debug_clip_slice_values (int n_channels);   /* clip batches: values of one padded slice, 3 (block frames + 5) 1024 C with the parameters in force */
int  awm_debug_clip_stage_d (awm_ctx *ctx, size_t n_clips, const float *const *pcm_d, const size_t *n_frames, int n_channels, int sample_rate,
                             float *slices_d, long long *range_out);
                                           /* stage 0 of a group alone: the padded slices of 1 .. 64 short clips into slices_d (n_clips x slice values, 16-byte aligned) on the
                                            * context's stream, their non-silent ranges to range_out (host, [n_clips][2]), synchronised.  44100: the padded copy; a rate of the
                                            * fixed-ratio Resampler: resampled into the slices.  AWM_ERR_ARG: a VResampler rate, a clip that is not short, more than 64 clips.  Honours
                                            * awm_debug_set_clip_poison */
int  awm_debug_clip_stage_rates_d (awm_ctx *ctx, size_t n_clips, const float *const *pcm_d, const size_t *n_frames, int n_channels,
                                   const int *sample_rates, float *slices_d, long long *range_out);
                                           /* its twin with a rate per clip: every clip with the form of its own rate (one launch per form present).
                                            * The same refusals, and those of awm_get_watermark_batch_rates_d */
int  awm_debug_clip_stage_rates_s16_d (awm_ctx *ctx, size_t n_clips, const int16_t *const *pcm_d, const size_t *n_frames, int n_channels,
                                       const int *sample_rates, float *slices_d, long long *range_out);
                                           /* ... and on 16-bit clips (awm_get_watermark_batch_rates_s16_d; sample_rates NULL: all at 44100): slices and ranges are bit for
                                            * bit those of awm_debug_clip_stage_rates_d on the decoded clips.  The same refusals, and an odd or (with frames) NULL pcm_d[i] */
void awm_debug_clip_form_launches (long out[3]); /* clip batches: stage 0 kernels launched by this process so far, by form: [0] generic taps, [1] phase per thread, [2] copy (the
                                            * profiling scopes count a group's stage 0 as one launch whatever its forms) */
size_t awm_debug_lane_pcm_bytes (awm_ctx *ctx); /* bytes the context's lanes hold as float copies of 16-bit clips (long clips, VResampler rates, speed search): 0 after
                                            * awm_ctx_trim and for as long as the 16-bit batches see short clips only */
size_t awm_debug_lane_add_mix_bytes (awm_ctx *ctx); /* bytes the context's lanes hold as the float mix of awm_add_watermark_s16_d (through the definition: its float result;
                                            * the decoded input counts under awm_debug_lane_pcm_bytes): 0 after awm_ctx_trim */
void awm_debug_set_clip_pad_margin (int frames); /* clip batches: frames of zeros written on either side of a clip (default and minimum 2048; one slice = 6693 frames
                                            * or more: whole slices, the A side of the measurement in tools/gpu_clip_margin_ab.py) */
void awm_debug_set_staged_threads (int n);  /* clip batches: host threads (= lanes) working on groups of clips; 0 = default (4; 2 with a key per clip only where the
                                            * tables cannot come from the device and host threads build them) */
void awm_debug_clip_key_timing (double us_out[3]); /* get with a key per clip, summed over the batch's host threads since the last call: [0] microseconds waiting for
                                            * a group's key tables (built on host threads one group ahead), [1] packing + uploading them, [2] groups */
double awm_debug_time_group_key_tables (int n_keys, int threads); /* host only: wall milliseconds the key tables of one group of n_keys clips take to build
                                            * (threads <= 0: 64 as shipped) */
void awm_debug_set_group_fallback (int on); /* clip batches: every clip takes the sequential peak selection on its own slice (normally the rare clips whose peak
                                            * lists overflow the grouped selection) */
void awm_debug_alloc_stats (long *dev_allocs, double *dev_ms, long *pinned_allocs, double *pinned_ms);
                                           /* process-wide census of hipMalloc / hipHostMalloc calls made by the library's grow-only buffers and the
                                            * time the runtime took for them (what a first call pays); any pointer may be NULL */
unsigned long long awm_debug_alloc_bytes (void);   /* ... and the device bytes those buffers asked hipMalloc for, summed over the process's life */
void awm_debug_file_timing (double ms_out[8]);
                                           /* where the calling thread's time went in its last file level `add` at the watermark rate (milliseconds):
                                            * [0] set-up (add stream, rings), [1] waiting for input tiles, [2] waiting for a free output slot, [3] queueing GPU
                                            * work, [4] the final wait for the GPU, [5] the final wait for the writers, [6] tear-down, [7] handing output tiles on
                                            * (includes [2]) */
void awm_debug_set_io_flags (int flags);   /* file level add / get, host side (host/wmfile.cc): bit 0 regular INPUT files are read by the I/O workers through the
                                            * stream's raw_region (else one reader thread in stream order, as for pipes) | bit 3 regular OUTPUT files of known
                                            * length are written by the workers (else one writer thread in stream order) -- then bit 1: through ONE shared mapping
                                            * of the file (else pwrite per part), bit 2: MADV_POPULATE_WRITE before the copy.  Default 1: creating the pages of
                                            * one file is serial in the kernel, the writer thread is at that floor (profiles/r05/io_probe.txt); the bytes written
                                            * are the same either way. */

/* Host threads that copy between the page cache and the page-locked staging rings of the file level calls (awm_add_watermark_file,
 * awm_get_watermark_file, the command line): 0 (default) = min (16, cores); one pool per process.  The reference reads and writes on
 * its one thread (wavchunkloader.cc:196-222, rawconverter.cc, stdoutwavoutputstream.cc). */
void awm_set_io_threads (int n);

/* --quiet (reference audiowmark.cc:1020-1023): the "Input: / Output: / Message: ..." information lines of add_watermark off */
void awm_set_quiet (int quiet);

/* ---- parameters (reference Params, wmcommon.hh:33-89) ------------------------------------------------------------------
 * The reference keeps its settings in static members of Params: one set per process.  This library has one process-wide set
 * with the same names and defaults -- awm_set_params / awm_set_speed_params / awm_set_global_params change it -- and every
 * context may carry its OWN set (awm_ctx_set_params), which is in force for all work entered through that context, also on the
 * helper threads the library starts for it.  Two contexts with different strength / thresholds / --hard can therefore work side
 * by side in one process; a context without its own set follows the process-wide one as of each call. */
void awm_set_params (double water_delta, int mix, int frames_per_bit, int test_no_limiter,
                     double sync_threshold2, int n_best, double chunk_size_min);
typedef struct
{
  size_t struct_size;            /* sizeof (awm_params), filled by awm_params_init / awm_ctx_get_params */
  double water_delta;            /* --strength / 1000            (Params::water_delta, default 0.01) */
  int    mix;                    /* 0 = --linear                 (Params::mix, 1) */
  int    hard;                   /* --hard: hard decode bits     (Params::hard, 0; wmget.cc:40-65) */
  int    strict;                 /* --strict: message length must equal payload_size, `add` refuses clipped input (Params::strict, 0) */
  int    snr;                    /* --snr: `add` reports the SNR (Params::snr, 0; file level only) */
  int    payload_size;           /* bits (Params::payload_size, 128; other sizes are refused by the compute entry points) */
  int    frames_per_bit;         /* (Params::frames_per_bit, 2: --frames-per-bit, reference audiowmark.cc:675; the compute entry points take 1 .. 8) */
  double sync_threshold2;        /* --sync-threshold (Params::sync_threshold2, 0.35) */
  int    get_n_best;             /* (Params::get_n_best, 8) */
  double get_chunk_size;         /* --chunk-size, minutes (Params::get_chunk_size, 30) */
  int    detect_speed, detect_speed_patient;   /* --detect-speed, --detect-speed-patient */
  double try_speed, test_speed;  /* --try-speed, --test-speed (-1: unset) */
  int    test_cut, test_no_sync, test_no_limiter, test_truncate;     /* the reference's --test-* knobs */
} awm_params;
void awm_params_init (awm_params *p);                               /* the reference's defaults */
int  awm_set_global_params (const awm_params *p);                   /* the process-wide set */
int  awm_ctx_set_params (awm_ctx *ctx, const awm_params *p);        /* p == NULL: back to the process-wide set */
int  awm_ctx_get_params (const awm_ctx *ctx, awm_params *out);      /* the set in force for ctx (ctx == NULL: the process-wide one) */

/* `add --snr` (reference wmadd.cc:553-563, 591-592): between begin and end every `add` of the context accumulates the power of its
 * input and of the watermark signal (mix - input, BEFORE the limiter, sums in double); SNR = 10 log10 (signal / delta). */
int  awm_ctx_snr_begin (awm_ctx *ctx);
int  awm_ctx_snr_end (awm_ctx *ctx, double *signal_power, double *delta_power);

#ifdef __cplusplus
}
#endif
#endif /* AWM_HIP_H */
