// kernels.hh -- host-callable launchers of the gfx950 kernels (kernels.hip, viterbi.hip).
// Everything here works on device pointers and enqueues on the given stream.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

// The kernels are written for ONE target.  They rely on gfx950's 160 KB of LDS per workgroup (K16: 117 KB static, K5w's ring 150 KB),
// on `sc1` device-coherent loads / stores with `s_waitcnt vmcnt(0)` for the cross-XCD meetings of the one-launch Viterbi kernel, on
// `global_load_lds_dwordx4` and on gfx9 buffer descriptors (K14).  Another --offload-arch must not build silently.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "audiowmark_amd's HIP kernels are written for gfx950 (MI355X) only"
#endif

namespace awmk {

// constant tables resident in HBM for the lifetime of a context
struct DevTables
{
  const float2 *tw512;    // e^{-2 pi i k / 512},  k < 512
  const float2 *tw1024;   // e^{-2 pi i k / 1024}, k <= 512
  const float  *window;   // normalised von Hann analysis window, 1024 (reference wmcommon.cc:68-89)
  const float  *synth;    // synthesis window, 3072 (reference wmadd.cc:177-206)
  const double2 *slide;   // [84 bins 19..102][9]: e^{-2 pi i k j / 1024}, j = 0..7, and e^{+2 pi i 8 k / 1024} at j = 8
  const double2 *tw512d;  // e^{-2 pi i k / 512} in double (first transform of a refinement row)
  const float2 *slide32;  // [84 bins 19..102][8]: e^{-2 pi i k j / 1024} e^{+2 pi i 8 k / 1024}, j = 0..7, rounded to float (K4s with the update term in float)
};

/* K1: FFTAnalyzer::run_fft / fft_range */
hipError_t launch_stft_full (hipStream_t st, const DevTables& t, const float *pcm, int n_channels,
                             long long start_index, long long hop, long long frame_count, float2 *out);

/* K2: fused STFT -> band edit -> inverse -> overlap-add -> mix (+ per-limiter-block maxima) */
struct AddMixArgs
{
  const float *pcm_in;
  float       *out;
  long long    n_frames;          // samples per channel in this span
  int          n_channels;
  const int8_t *frame_mod;        // device, [4452][81]
  float        neg_delta_up;      // (float) (-water_delta * +1)
  float        neg_delta_down;    // (float) (-water_delta * -1)
  long long    first_frame;       // global frame index of local frame 0
  const float *halo_before;       // 1024*C samples or nullptr
  const float *halo_after;        // 1024*C samples or nullptr
  unsigned int *block_max;        // float bits, or nullptr
  long long    first_block;
  long long    n_blocks;
  int          limiter_block;     // samples per limiter block (44100)
  int          frames_per_span;   // frames each wave streams through
  int          block_frames = 2226;   // mark_block_frame_count(): sync + data frames of a block (wmcommon.cc:36-48)
  int          frames_pad_start = 250; // Params::frames_pad_start
  int          delta_only = 0;    // 1: write the watermark signal alone (out = d W..., without "+ in"): WatermarkGen::run for the resampled path
};
hipError_t launch_add_mix (hipStream_t st, const DevTables& t, const AddMixArgs& a);
/* a batch of STEREO clips in one launch: args_dev[n_clips] on the device (every clip a stream of its own: first_frame 0, no halos, its own
 * block_max), max_spans = the largest ceil (ceil (n_frames / 1024) / frames_per_span) among them; block_frames / frames_pad_start as in the arguments */
hipError_t launch_add_mix_batch (hipStream_t st, const DevTables& t, const AddMixArgs *args_dev, int n_clips, long long max_spans, int block_frames,
                                 int frames_pad_start);
int        add_mix_waves_per_simd();     // occupancy the stereo kernel is built for (sizes the spans: one round of resident waves)

/* K2m: K2 for ONE input stream and several outputs, each with a frame_mod table of its own (one programme, one payload per recipient).
 * A wave fetches, windows and transforms a frame once and computes both band factors (UP and DOWN) once; band selection, inverse
 * transform, overlap-add, mix, stores and block maxima then run once per output.  This form: whole streams (frame 0 is sample 0, no halos; spans: AddMixSpan below);
 * every channel count takes it (stereo through the paired transforms, anything else one channel per wave like K2).  out[p] is bit for bit
 * what launch_add_mix writes with frame_mod[p]: both kernels call the same device functions for every step after the band edit. */
constexpr int ADD_MULTI_TILE = 4;        // outputs per launch (their overlap-add carry lives in registers: DESIGN.md section 9)
struct AddMixOut
{
  float        *out;
  const int8_t *frame_mod;        // device, [2 * block_frames][81]
  unsigned int *block_max;        // float bits, n_blocks of them, or nullptr
};
struct AddMixMultiArgs
{
  const float *pcm_in;
  long long    n_frames;          // samples per channel
  int          n_channels;
  float        neg_delta_up;      // as in AddMixArgs
  float        neg_delta_down;
  long long    n_blocks;
  int          limiter_block;
  int          frames_per_span;
  int          block_frames;
  int          frames_pad_start;
  int          n_out;             // 1 .. ADD_MULTI_TILE
  AddMixOut    o[ADD_MULTI_TILE];
  int          delta_only = 0;    // as in AddMixArgs: every output receives the watermark signal alone (the stream at another sample rate)
};
hipError_t launch_add_mix_multi (hipStream_t st, const DevTables& t, const AddMixMultiArgs& a);
int        add_mix_multi_waves_per_simd();   // occupancy K2m is built for (sizes its spans)
/* K2m for a SPAN of a stream (the P-output form of AddMixArgs' span fields, with add_mix_body's meaning): local frame m is frame
 * first_frame + m of the stream (table row, limiter block), frame -1 / frame ceil (n_frames / 1024) come from the halos (nullptr: zeros),
 * block maxima are stored at index - first_block (o[p].block_max has n_blocks entries from there).  The halo frames are transformed once
 * per launch like every other frame.  out[p] is bit for bit what launch_add_mix writes for the span with frame_mod[p]. */
struct AddMixSpan
{
  long long    first_frame;       // global frame index of local frame 0
  const float *halo_before;       // 1024*C samples or nullptr
  const float *halo_after;        // 1024*C samples or nullptr
  long long    first_block;
};
hipError_t launch_add_mix_multi_span (hipStream_t st, const DevTables& t, const AddMixMultiArgs& a, const AddMixSpan& sp);
int        add_mix_multi_span_waves_per_simd();   // occupancy the span kernels are built for

/* K3: limiter ramp, in place */
hipError_t launch_limiter (hipStream_t st, float *data, long long n_frames, int n_channels, long long first_sample,
                           const float *block_max, long long first_block, long long n_blocks,
                           int limiter_block, float ceiling, float2 *scale_tab = nullptr, size_t scale_tab_entries = 0);
/* K3 for a batch of clips (1 or 2 channels, data 16 byte aligned), every clip a stream of its own with its own block maxima and a ramp
 * table of limiter_tab_entries (n_frames, first_sample, limiter_block) entries: two launches for the batch.  first_sample / first_block
 * have launch_limiter's meaning (data[0] is sample first_sample of the clip's stream, block_max[0] the maximum of limiter block
 * first_block); 0 / 0: a stream that starts at sample 0.  max_tab: the largest n_tab among the clips (0: what max_frames gives for
 * first_sample 0). */
struct LimiterClip
{
  float *data; long long n_frames; const float *block_max; long long n_blocks; float2 *tab; long long n_tab;
  long long first_sample, first_block;       // (a brace list that ends before them leaves both 0)
};
/* gather / scatter of a batch of interleaved STEREO segments in one launch (float2 pieces: src, dst + zeros and the counts are whole
 * frames from 16-byte aligned bases): dst[0 .. zeros) = 0, dst[zeros .. zeros + n_values) = src[0 .. n_values).  n_values 0: nothing. */
struct SegmentCopy { const float *src; float *dst; long long n_values, zeros; };
hipError_t launch_segment_copy (hipStream_t st, const SegmentCopy *copies_dev, int n_copies, long long max_values);
hipError_t launch_limiter_batch (hipStream_t st, const LimiterClip *clips_dev, int n_clips, long long max_frames, int n_channels, int limiter_block,
                                 float ceiling, long long max_tab = 0);
/* the first of launch_limiter_batch's two launches alone: the ramp tables of the clips (data and n_frames are not read) */
hipError_t launch_limiter_table_batch (hipStream_t st, const LimiterClip *clips_dev, int n_clips, long long max_frames, int limiter_block, float ceiling,
                                       long long max_tab = 0);
/* The 16-BIT SEGMENT BATCHES (awm_add_watermark_segments_rate_s16_d): signed 16-bit PCM, little-endian, interleaved stereo, every address
 * 4-byte aligned (a stereo frame is one load or store).
 * launch_segment_gather_s16: launch_segment_copy whose sources are int16 -- `src` holds their ADDRESS --, decoded as launch_pcm_decode
 * decodes them, float (v) * (1 / 32768): dst[0 .. zeros) = 0, dst[zeros .. zeros + n_values) = the decoded values.
 * launch_limit_encode_segments: limiter ramp and encode in one pass over a batch of segments, blockIdx.y = segment.  The un-limited mix of
 * frame f is wm[f] (mix false) or wm[f] + the decoded orig[f] (mix true: launch_mix_max_segments' add, nothing of it was stored; `orig`
 * holds the address of the segment's int16 values); it is multiplied by the ramp launch_limiter_batch applies -- tab[b - tab_first_block]
 * is the (scale_start, scale_step) of limiter block b, frame f is sample first_sample + f of its stream; tab null: no ramp -- and goes
 * through launch_pcm_encode's direct16 rule (v * 32768, saturated at 32767 / -32768, truncated) to out[f].  out is bit for bit what
 * launch_limiter_batch over the stored mix and launch_pcm_encode write.  Nothing outside out[0 .. 2 n_frames) is written: 16-byte stores
 * from the first 16-byte boundary of out, single frames in front and behind.  limiter_block >= 2048. */
hipError_t launch_segment_gather_s16 (hipStream_t st, const SegmentCopy *copies_dev, int n_copies, long long max_values);
struct LimitEncodeSegment
{
  const void   *orig;
  const float  *wm;
  short        *out;
  long long     n_frames, first_sample;
  const float2 *tab;
  long long     tab_first_block;
};
hipError_t launch_limit_encode_segments (hipStream_t st, const LimitEncodeSegment *segs_dev, int n_segs, long long max_frames, bool mix, int limiter_block);
/* entries launch_limiter needs in scale_tab for this span (one (scale_start, scale_step) pair per limiter block) */
size_t     limiter_tab_entries (long long n_frames, long long first_sample, int limiter_block);
hipError_t launch_fill_u32 (hipStream_t st, unsigned int *p, unsigned int v, size_t n);

/* K10: fixed-ratio polyphase resampler = zita-resampler's Resampler (restated; the reference uses it with hlen 16 for
 * every sample rate other than 44100 Hz, resample.cc:128-270).  Output frame m of the stream "hl - 1 null frames, the
 * input, null frames for ever":  b = floor (m s / np), ph = m s mod np,
 *   y[m] = (1e-20f + sum_{i < hl} (P[b + i] c1[i] + P[b + 2 hl - 1 - i] c2[i])) - 1e-20f,   c1 = ctab + hl ph, c2 = ctab + hl (np - ph)
 * in float, products and sums rounded separately in this order. */
struct ResampleArgs
{
  const float *in;
  long long    n_in;        // frames available (everything else reads as zero)
  int          n_channels;
  const float *ctab;        // device, (np + 1) * hl
  int          hl, np, step; // step = s = fs_in / gcd
  float       *out;
  long long    n_out;       // frames to produce
};
hipError_t launch_resample (hipStream_t st, const ResampleArgs& a);
/* K10w: K10 for WINDOWS of streams, a batch of them in one launch (blockIdx.y = slice, its arguments from an array on the device).  A slice
 * is a run of outputs of one stream and the part of that stream's input that is resident: output out0 + k (k < n_out) goes to out[k], input
 * frame j of the stream is in[j - in0] for in0 <= j < in0 + n_in and reads as zero everywhere else.  Window start, phase, products and sums
 * are K10's for the GLOBAL output index (m step in 64 bits: m < 2^41 and step <= 16000, see awm_add_segment_plan); ctab / hl / np / step /
 * n_channels come from `a`, whose in / out fields are not read.  Stereo with every pointer 8-byte aligned (stereo_aligned) stages the
 * tile's window in LDS like K10; everything else takes the generic taps. */
struct ResampleSlice
{
  const float *in;
  long long    n_in, in0;
  long long    out0, n_out;
  float       *out;
};
hipError_t launch_resample_slices (hipStream_t st, const ResampleArgs& a, const ResampleSlice *slices_dev, int n_slices, long long max_n_out,
                                   bool stereo_aligned);
hipError_t launch_resample_slice (hipStream_t st, const ResampleArgs& a, const ResampleSlice& slice);     // one slice, arguments by value
/* K10w over slices whose input is SIGNED 16-BIT PCM (the kernels instantiated for PcmS16, like stage 0 of the clip groups: `in` holds the
 * ADDRESS of the int16 values, a value is converted once, where it leaves global memory): out is bit for bit what launch_resample_slices
 * writes for the decoded input.  stereo_aligned: every input 4-byte aligned, every output 8-byte aligned */
hipError_t launch_resample_slices_s16 (hipStream_t st, const ResampleArgs& a, const ResampleSlice *slices_dev, int n_slices, long long max_n_out,
                                       bool stereo_aligned);
/* K10s: one slice whose caller chooses where it begins (the tile stream at another rate, which ends every launch on a multiple of np and
 * carries the rest).  Stereo 48 <-> 44.1 kHz with every pointer 8-byte aligned, out0 a multiple of np and awm_debug_set_resample_phase on
 * runs K10's phase-per-thread body at the slice's place in its stream (resample_span_takes_phase says whether); everything else is
 * launch_resample_slice.  The bits are the same either way. */
bool       resample_span_takes_phase (const ResampleArgs& a, const ResampleSlice& slice);
hipError_t launch_resample_span (hipStream_t st, ResampleArgs a, ResampleSlice slice);

/* K10m: K10 on the way up (44.1 -> 48 kHz: np 160, step 147, hl 16) for the watermark signals of up to ADD_MULTI_TILE outputs of ONE
 * stereo stream, fused with K11: out[o][m] = K10's output m of wm44[o] + orig[m], one rounded add, and block_max[o] receives the maxima of
 * |out[o]| per limiter block (float bits, atomicMax; nullptr: none).  A thread owns a phase: its coefficients stay in registers for the
 * launch, the samples of orig that it adds to for a tile's outputs.  out[o] is bit for bit what launch_resample into a buffer and
 * launch_mix_max from it write, and so are the maxima.  Every pointer 8-byte aligned, limiter_block >= 2560 (the tile):
 * resample_mix_multi_takes says whether a call qualifies, the launcher refuses what does not. */
struct ResampleMixOut
{
  const float  *wm44;       // the output's watermark signal at 44.1 kHz, n_in frames (everything else reads as zero)
  float        *out;        // n_out frames
  unsigned int *block_max;  // n_blocks maxima from limiter block 0, or nullptr
};
struct ResampleMixArgs
{
  const float *orig;        // the stream at the rate, n_out frames
  long long    n_in;
  int          n_channels;
  const float *ctab;        // device, (np + 1) * hl
  int          hl, np, step;
  long long    n_out;
  long long    n_blocks;
  int          limiter_block;
  int          n;           // 1 .. ADD_MULTI_TILE
  ResampleMixOut o[ADD_MULTI_TILE];
};
bool       resample_mix_multi_takes (const ResampleMixArgs& a);
hipError_t launch_resample_mix_multi (hipStream_t st, const ResampleMixArgs& a);

/* K11: out = wm + orig (reference wmadd.cc:564-565) and the per-limiter-block maxima of the result (limiter.cc:90-97) */
hipError_t launch_mix_max (hipStream_t st, const float *orig, const float *wm, float *out, long long n_frames, int n_channels,
                           unsigned int *block_max, long long n_blocks, int limiter_block);
/* K11 for a batch of stream segments (blockIdx.y = segment): out[0 .. n_frames) = wm[pre ..] + orig, where orig[0] / out[0] are sample
 * first_sample of the segment's stream and wm[0] is sample first_sample - pre of the watermark signal.  The `pre` samples in front are
 * watermark alone (the stream is silent there): nothing is stored for them, but they count for the block maxima like the rest.
 * block_max[0] belongs to limiter block first_block (nullptr: no maxima). */
struct MixSegment
{
  const float  *orig, *wm;
  float        *out;
  long long     n_frames, pre, first_sample;
  unsigned int *block_max;
  long long     first_block, n_blocks;
};
hipError_t launch_mix_max_segments (hipStream_t st, const MixSegment *segs_dev, int n_segs, long long max_frames, int n_channels, int limiter_block);
hipError_t launch_mix_max_segment (hipStream_t st, const MixSegment& seg, int n_channels, int limiter_block);   // one segment, arguments by value
/* the block maxima of launch_mix_max_segments ALONE, for segments of signed 16-bit PCM (`orig` holds the address of the int16 values,
 * decoded as they are read): the same add, the same maxima, `out` is not read or written */
hipError_t launch_max_segments_s16 (hipStream_t st, const MixSegment *segs_dev, int n_segs, long long max_frames, int n_channels, int limiter_block);

/* The SEGMENT BATCHES WITH A RATE PER SEGMENT (awm_add_watermark_segments_rates_d): the launchers above whose
 * launch-uniform rate-dependent argument -- the resampler's geometry, the limiter block -- comes from the descriptor of blockIdx.y instead.
 * Each descriptor is the one-rate descriptor and the rate's values behind it; each kernel reads them once per workgroup (uniform: scalar
 * registers) and runs the body of its one-rate kernel, so slice / segment i is bit for bit what the one-rate launcher writes for it with
 * that rate's arguments.  Grids are sized by the longest slice / segment / ramp table of the batch, the launchers' lower bounds on the
 * limiter block hold for min_limiter_block, the smallest of the batch.
 * K10w: ctab / hl / np / step of the slice's table (down: rate -> 44.1 kHz, up: 44.1 kHz -> rate), lds_floats = floats of the table in LDS
 * or 0 (taps from global memory), in_span = frames of the tile's window or 0 (not staged) -- resample_slice_geometry fills both as
 * launch_resample_slices decides for a launch at that rate.  Dynamic LDS is the largest table + window among the slices (lds_bytes: the
 * maximum of resample_slice_lds_bytes over them). */
struct RateResampleSlice
{
  ResampleSlice s;
  const float  *ctab;
  int           hl, np, step;
  int           lds_floats, in_span;
};
void       resample_slice_geometry (RateResampleSlice& r /* ctab, hl, np, step set */, int n_channels, bool stereo_aligned);
size_t     resample_slice_lds_bytes (const RateResampleSlice& r);
hipError_t launch_resample_slices_rates (hipStream_t st, const RateResampleSlice *slices_dev, int n_slices, int n_channels, long long max_n_out,
                                         bool stereo_aligned, size_t lds_bytes);
hipError_t launch_resample_slices_rates_s16 (hipStream_t st, const RateResampleSlice *slices_dev, int n_slices, int n_channels, long long max_n_out,
                                             bool stereo_aligned, size_t lds_bytes);
struct RateMixSegment { MixSegment s; int limiter_block; };
hipError_t launch_mix_max_segments_rates (hipStream_t st, const RateMixSegment *segs_dev, int n_segs, long long max_frames, int n_channels,
                                          int min_limiter_block);
hipError_t launch_max_segments_rates_s16 (hipStream_t st, const RateMixSegment *segs_dev, int n_segs, long long max_frames, int n_channels,
                                          int min_limiter_block);
struct RateLimiterClip { LimiterClip c; int limiter_block; };
hipError_t launch_limiter_table_batch_rates (hipStream_t st, const RateLimiterClip *clips_dev, int n_clips, float ceiling, long long max_tab);
hipError_t launch_limiter_batch_rates (hipStream_t st, const RateLimiterClip *clips_dev, int n_clips, long long max_frames, int n_channels,
                                       int min_limiter_block, float ceiling, long long max_tab);
struct RateLimitEncodeSegment { LimitEncodeSegment s; int limiter_block; };
hipError_t launch_limit_encode_segments_rates (hipStream_t st, const RateLimitEncodeSegment *segs_dev, int n_segs, long long max_frames, bool mix,
                                               int min_limiter_block);

/* `add --snr`: acc[0] += sum (mixed - orig)^2, acc[1] += sum orig^2 in double (reference wmadd.cc:553-563) */
hipError_t launch_power_sums (hipStream_t st, const float *orig, const float *mixed, long long n_values, double *acc);

/* K4: STFT -> dB of the 81 bands, written band-major ("transposed") so that scans over the
 * frame axis are coalesced.  Stream s (0 <= s < n_streams) consists of count(s) frames starting
 * at base(s) + f * hop.  out[s * out_stream_stride + (plane * 81 + band) * ld + f]. */
struct SyncDbArgs
{
  const float *pcm;
  long long    n_frames;          // samples per channel available (bounds)
  int          n_channels;
  int          per_channel;       // 0: channels summed into one plane; 1: one plane per channel
  long long    base0, base_stride;      // base(s) = base0 + s * base_stride     (if stream_base == nullptr)
  const long long *stream_base;         // device array [n_streams] or nullptr
  int          count0;                  // count(s) = count0                      (if stream_count == nullptr)
  const int   *stream_count;            // device array [n_streams] or nullptr
  long long    n_streams;
  long long    hop;
  float       *out;
  long long    out_stream_stride;
  long long    ld;
  char        *have;                    // have[s * have_stream_stride + f] or nullptr
  long long    have_stream_stride;
  long long    first, last;             // non-silent value range [first, last) (syncfinder.cc:155-169)
  int          tile_frames;             // frames per workgroup tile (<= 72)
  int          xcd_interleave = 0;      // set by the launcher: 1-D grid, the streams of one tile on the same XCD (see kernels.hip)
  // K4s only, "gathered" output for the refinement scan (K5g): stream s = plane * rows_per_plane + w writes its
  // rows to stream slot plane * rows_per_plane + row_perm[w], and band b to row band_pos[w * 81 + b] (255: dropped)
  const int           *row_perm = nullptr;
  const unsigned char *band_pos = nullptr;
  int                  rows_per_plane = 0;
  // ... and, with forms 4 / 5 of K4s, the rows' 65th value (fine offset 64) apart from the rows: tail[slot * tail_stream_stride + row],
  // so that a row of `ld` = 64 floats is two whole cache lines (nullptr: offset 64 goes into the row like the others, ld >= 65)
  float               *tail = nullptr;
  long long            tail_stream_stride = 0;
  // a batch of clips with one KEY PER CLIP: the tables of slice i (range_index / range_div as below) follow those of slice i - 1:
  // row_perm + slice * rows_per_plane, band_pos + slice * rows_per_plane * 81
  int                  tables_per_slice = 0;
  // Slices (the batched clip search: many padded clips side by side in one buffer).  With streams_per_slice > 0 stream s is
  // stream s % streams_per_slice of slice s / streams_per_slice: base = base0 + (s % sps) * base_stride + (s / sps) * slice_stride.
  // stream_range, if set, replaces first / last by the range of the stream's slice: slice = range_index[s / range_div] if
  // range_index is set, else s / range_div; entries are absolute value indices [first, last), first < 0 = nothing but silence.
  int                  streams_per_slice = 0;
  long long            slice_stride = 0;
  const long long     *stream_range = nullptr;
  const int           *range_index = nullptr;
  int                  range_div = 1;
  // 1: a frame in the silence outside the range is not skipped but gets the dB values of a transformed frame of zeros (exactly
  // what the transform would deliver: -96 per band and channel) -- the block decoder's fft_range knows no skipping
  int                  silent_frames_are_zero = 0;
  // with silent_frames_are_zero: a tile all of whose frames, and the two frames on either side of it, lie in that silence is not
  // written at all -- for the one consumer that never reads such frames (K7 with SoftBitsArgs::stream_range)
  int                  skip_unread_silent_tiles = 0;
};
hipError_t launch_sync_db (hipStream_t st, const DevTables& t, const SyncDbArgs& a);
/* K4s: same output as K4 for streams whose frames advance by 8 samples (search_refine): instead of one FFT per fine
 * offset the 83 needed bins are carried from offset to offset by a sliding DFT in double precision. n_channels <= 2. */
hipError_t launch_sync_db_sliding (hipStream_t st, const DevTables& t, const SyncDbArgs& a);
/* does the form of K4s in force (awm_debug_set_refine_form) write rows of 64 fine offsets + SyncDbArgs::tail for streams of this many channels? */
bool sliding_rows_have_tail (int n_channels);

/* WHOLE STREAMS OF SIGNED 16-BIT PCM (awm_get_watermark_s16_d and its twins): K4, K4b, K4s, the silence scan and the fixed-ratio resampler
 * instantiated for PcmS16.  The args are the float launchers' -- SyncDbArgs::pcm / ResampleArgs::in hold the ADDRESS of the int16 values,
 * interleaved, little-endian, any even address (odd: hipErrorInvalidValue) -- and every output is bit for bit what the float launcher
 * writes for the decoded stream, float (v) * (1 / 32768) (launch_pcm_decode): a value is converted once, where it leaves global memory,
 * and nothing behind the load differs.  Stereo frames that are 4-byte aligned are loaded whole; a stereo stream on an address that is
 * only 2-byte aligned and mono streams off a 4-byte boundary take 2-byte loads.  Nothing outside the stream's values is read.
 * launch_sync_db_sliding_s16 has the DEFAULT forms only (stereo: form 4 with gathered rows, band_pos set; mono: sync_db_sliding_kernel<1>):
 * hipErrorInvalidValue while awm_debug_set_refine_form selects another one (sliding_s16_form_ok). */
hipError_t launch_sync_db_s16 (hipStream_t st, const DevTables& t, const SyncDbArgs& a);
hipError_t launch_sync_db_sliding_s16 (hipStream_t st, const DevTables& t, const SyncDbArgs& a);
bool sliding_s16_form_ok();
hipError_t launch_nonzero_range_s16 (hipStream_t st, const int16_t *data, long long n_values, unsigned long long *result);
hipError_t launch_resample_s16 (hipStream_t st, const ResampleArgs& a);

/* WHOLE STREAMS FROM AND TO SIGNED 16-BIT PCM (awm_add_watermark_s16_d).
 * launch_add_mix_s16: K2 instantiated for PcmS16, the span form included.  AddMixArgs::pcm_in, halo_before and halo_after hold the ADDRESS
 * of int16 values (interleaved, any even address; odd: hipErrorInvalidValue), converted where they leave global memory; out and block_max
 * are bit for bit what launch_add_mix writes for the decoded stream and the decoded halos.
 * launch_limit_encode: the last pass, launch_limiter's arguments plus the int16 sink.  out[v] is the direct16 rule of launch_pcm_encode
 * (v * 32768, saturated at 32767 / -32768, truncated) of what launch_limiter leaves of mix[v]; mix is not modified and nothing outside
 * out[0 .. n_frames * n_channels) is written.  block_max null: no ramp.  Stereo on a 4-byte aligned sink (mix 8-byte aligned): groups of
 * four frames, one 16-byte store each (limit_encode_segment_body); mono: groups of eight values; every other channel count, a stereo sink
 * that is only 2-byte aligned, limiter blocks below 2048 and a missing table workspace: a value per thread with launch_limiter's generic
 * arithmetic.  No run is skipped where its ramp is (1, 0).  orig (stereo vector form only, else hipErrorInvalidValue): the address of
 * int16 frames, 4-byte aligned; the value is mix[v] + the decoded orig[v] (launch_max_segment_s16's add), and a frame of orig is read for the
 * last time by the thread that stores the same frame of out, so out may BE orig.
 * launch_max_segment_s16: launch_max_segments_s16 for one segment, arguments by value. */
hipError_t launch_add_mix_s16 (hipStream_t st, const DevTables& t, const AddMixArgs& a);
hipError_t launch_limit_encode (hipStream_t st, const float *mix, short *out, long long n_frames, int n_channels, long long first_sample,
                                const float *block_max, long long first_block, long long n_blocks, int limiter_block, float ceiling,
                                float2 *scale_tab = nullptr, size_t scale_tab_entries = 0, const void *orig = nullptr);
hipError_t launch_max_segment_s16 (hipStream_t st, const MixSegment& seg, int n_channels, int limiter_block);
hipError_t launch_power_sums_s16 (hipStream_t st, const int16_t *orig, const float *mixed, long long n_values, double *acc);   // launch_power_sums, the input decoded as it is read

/* K5: sync_decode (syncfinder.cc:116-153) for many candidates.
 * value(cand, row, band) = db[plane(cand) + row * row_stride + band * band_stride + lane(cand)],
 * have(cand, row)        = have[hplane(cand) + row * have_row_stride + lane(cand)]
 * where cand = group * 64 + lane-in-wave, plane(cand) = group_plane[...] see kernels.hip. */
struct SyncTableDev
{
  // [6][rows][64] int32: [0..29] up bands, [30..59] down bands (band - 20), [60] row index
  // (frame for the approximate search, want-list position for the refinement); wave-uniform -> scalar loads
  const int *packed;
  int        rows_per_bit;
  // K5w only (approximate search): [12 chains = sync bit x (up, down)][rows][8] words = the chain's 30 bands of the row as bytes,
  // then the frame of the chain's NEXT row as u16 (0xffff: none): one 32-byte scalar load per sync frame
  const unsigned *chains = nullptr;
  // a batch of clips with one key per clip: plane p uses the chains at chains + (p / planes_per_slice) * chains_slice_stride (words)
  long long       chains_slice_stride = 0;
  int             planes_per_slice = 1;
  // ... and the frame of every row, [slice][6][rows] (K5w in CLIP mode looks rows up by frame; one key: packed[..][60] serves)
  const int      *row_frames = nullptr;
};
/* host side of SyncTableDev::chains from a [6][rows][64] packed table */
void pack_scan_chains (const int *packed, int rows_per_bit, unsigned *out /* [12 * rows_per_bit * 8] */);
struct SyncScanArgs
{
  const float *db;
  const char  *have;            // nullptr: every frame present
  int          have_is_run = 0; // 1: the present frames of every plane form one run and absent frames hold +0 in db (what K4's silence rule
                                // produces): lets launch_sync_scan_window use the streaming kernel in CLIP mode too
  long long    plane_stride;    // between blockIdx.y planes (shifts / candidates)
  long long    have_plane_stride;
  long long    row_stride, band_stride, have_row_stride;
  long long    n_lanes;         // candidates per plane (start frames, or fine offsets)
  const int   *lane_count;      // optional per-plane valid lane count (refine), else n_lanes
  long long    n_planes;
  double       min_delta;       // min (water_delta, 0.080), reference syncfinder.cc:80-92
  double      *quality;         // [plane][q_stride]
  long long    q_stride;
  SyncTableDev table;
};
hipError_t launch_sync_scan (hipStream_t st, const SyncScanArgs& a);
/* K5w (scan.hip): same result for band-major planes (row_stride == 1, band_stride % 64 == 0, table.chains set): the dB
 * matrix streams through an LDS ring, four candidates per lane.  total_frames = frames a candidate spans (2226 BLOCK / 4452 CLIP). */
hipError_t launch_sync_scan_window (hipStream_t st, const SyncScanArgs& a, int total_frames);

/* K5g: sync_decode over the gathered layout K4s writes for the refinement: plane (candidate) p holds
 * [6 bits][rows_per_bit][60 values: up 0..29, down 0..29][ld fine offsets] -- exactly the order the sums consume them,
 * so the scan is a sequential stream without any table.  have: [plane][6 * rows_per_bit][ld] or nullptr. */
struct GatheredScanArgs
{
  const float *db;
  const char  *have;
  long long    plane_stride, have_plane_stride;
  int          ld;
  int          have_ld = 0;     // row length of `have` if it is not ld
  const float *tail = nullptr;  // K4s forms 4 / 5: the values of fine offsets >= ld (there is one: 64), [plane][6 bits][rows_per_bit][60]
  long long    tail_plane_stride = 0;
  int          rows_per_bit;
  int          n_lanes;         // fine offsets (<= 128)
  const int   *lane_count;      // per plane
  long long    n_planes;
  double       min_delta;
  double      *quality;         // [plane][q_stride]
  long long    q_stride;
  float       *chain_mag;       // scratch [plane][12 chains = (bit, up / down)][128]: the chains' sums
  int         *chain_n;         // scratch [plane][6 bits][128]: sync frames that counted
  int          regular_waves, tail_first, tail_lanes;     // set by the launcher
};
constexpr size_t GATHERED_SCRATCH_BYTES_PER_PLANE = 18 * 128 * 4;
hipError_t launch_sync_scan_gathered (hipStream_t st, const GatheredScanArgs& a);

/* K5b: local mean over the index-sorted scores (syncfinder.cc:234-254); q is [4][q_stride] by shift,
 * sorted position p = 4 * start_frame + shift.  Writes raw[p], mean[p]. */
/* n_slices > 1: slice y reads q + y * 4 * q_stride and writes raw_sorted / local_mean + y * 4 * n_start_frames */
hipError_t launch_local_mean (hipStream_t st, const double *q, long long q_stride, long long n_start_frames,
                              double *raw_sorted, double *local_mean, int n_slices = 1);

/* K5c: local maxima + false-positive mask + threshold on the device (syncfinder.cc:258-332, 364-383) */
struct PeakOut { long long p; double raw, mean; };
hipError_t launch_peak_select (hipStream_t st, const double *raw_sorted, const double *local_mean, long long n, double threshold,
                               unsigned int *count, PeakOut *out, unsigned int cap);
/* the same for n_slices independent score lists of n scores each: slice y uses raw / mean + y * n, the counter count[y * count_stride]
 * (NOT cleared here) and the list out + y * cap */
hipError_t launch_peak_select_slices (hipStream_t st, const double *raw_sorted, const double *local_mean, long long n, double threshold,
                                      unsigned int *count, int count_stride, PeakOut *out, unsigned int cap, int n_slices);

/* K5d: per-slice top k (by |raw - mean|) of a peak list whose length lives in *count; out is [n_slices][k], p = -1 = empty */
hipError_t launch_peak_topk (hipStream_t st, const PeakOut *in, const unsigned int *count, unsigned int cap, PeakOut *out, int k, int n_slices);
/* the same for n_lists lists: list y = in + y * cap with its length in count[y * count_stride], result out + y * n_slices * k */
hipError_t launch_peak_topk_lists (hipStream_t st, const PeakOut *in, const unsigned int *count, int count_stride, unsigned int cap,
                                   PeakOut *out, int k, int n_slices, int n_lists);

/* K7: mix_decode (wmget.cc:67-108): db is [n_blocks][C][81][ld] (band-major), out [n_blocks][858] */
struct SoftBitsArgs
{
  const float   *db;
  long long      block_stride, ld;
  int            n_channels;
  const int16_t *mix_frame;     // [n_entries]
  const uint8_t *mix_up, *mix_down;
  int            n_data_frames; // 1716
  int            frames_per_bit;
  int            block_frames;  // 2226
  long long      n_blocks;
  float         *out;
  // one key per clip: block b takes the mix table of slice block_slice[b] (entries at + slice * n_data_frames * 30)
  const int     *block_slice = nullptr;
  // Blocks cut out of padded slices (clip batches): block b starts at sample block_base[b] of the buffer; the values of its slice that are
  // not digital silence are [stream_range[2 s], stream_range[2 s + 1]) with s = range_index[b] (first < 0: nothing but silence) -- the
  // arrays K4b got (SyncDbArgs).  A frame outside that range has -96 dB in every band and channel (K4b writes exactly that,
  // silent_frames_are_zero), so an item whose frame AND both neighbours are such frames is known without a load: (-96, -192, -96, -192).
  // Four fifths of a 30 s clip's padded block are such items.  The sums are the same operations on the same values.
  const long long *block_base = nullptr;
  const long long *stream_range = nullptr;
  const int       *range_index = nullptr;
};
hipError_t launch_soft_bits (hipStream_t st, const SoftBitsArgs& a);
/* true if launch_soft_bits runs the kernel that takes the items in the padding's silence without a load (3+ channels at --frames-per-bit 3
 * and awm_debug_set_soft_bits_generic take the one that loads every cell: K4b must not leave any unwritten then) */
bool soft_bits_skips_silent_items (int n_channels, int frames_per_bit);

/* K7b: everything between mix_decode and the Viterbi decoder, per decode job (reference wmget.cc:40-65 normalize_soft_bits,
 * wmcommon.cc:165-185 randomize_bit_order, wmget.cc:554-701 AB interleave / "all" average): the raw soft bits of the
 * blocks never leave the device.  Job j reads its sources src[src_off .. src_off + n_src) = (block slot, half) and
 * writes len = 858 (single block) or 1716 normalised soft bits to out + out_off. */
struct SoftJobDev
{
  int       mode;          // 0: one block; 1: interleave (half 0 / 1 of every pair of bits); 2: average of several blocks per half
  int       n_src, src_off;
  int       len;           // 858 or 1716
  int       norm0, norm1;  // mode 2: blocks per half
  long long out_off;       // floats
  int       order_off;     // inv_order + order_off: the bit order of this job's key (one key per clip: n_bits * slice)
  int       pad;
};
struct SoftPrepArgs
{
  const float      *raw;         // [slots][n_bits]
  int               n_bits;      // 858
  const int        *inv_order;   // [n_bits]: restored[k] = raw[inv_order[k]]
  const SoftJobDev *jobs;
  const int2       *src;         // (slot, half)
  long long         n_jobs;
  int               hard;        // Params::hard
  float            *out;
};
hipError_t launch_soft_prep (hipStream_t st, const SoftPrepArgs& a);

/* K8: soft Viterbi (convcode.cc:128-213), one workgroup per coded block */
/* index 0 / 1 / 2 = A / B / AB coded blocks (rate 6 / 6 / 12); every block has n_steps = payload + 15 trellis steps */
/* sync_ws: viterbi_sync_bytes (all blocks of the call) bytes that are ZERO on entry and zero again when the launch has finished
 * (the one-launch kernel's tickets and per-decode counters; a lane keeps one such block and zeroes it when it allocates it);
 * nullptr: the chain of 16 launches.  A decode that reports error -2 means a device-side wait gave up: the batch is invalid. */
hipError_t launch_viterbi (hipStream_t st, const float *const soft[3], const long long n_blocks[3], long long n_steps,
                           unsigned char *const decisions_ws[3], int *const bits_out[3], float *const error_out[3], unsigned int *sync_ws);
size_t viterbi_workspace_bytes (long long coded_len, int rate, long long n_blocks);
bool viterbi_steps_supported (long long n_steps);  // 15 <= n_steps and a plan of at most 64 rounds: everything else is refused on the host
size_t viterbi_sync_bytes (long long n_blocks);
/* microseconds per launch of a chain of empty dependent launches on the (idle) stream: decides, per process, between the chain of 16
 * launches and the one-launch kernel (viterbi.hip) */
double probe_dependent_launch_us (hipStream_t st);
const char *viterbi_form_description();          // which form the batches take and why (for error messages)

/* K16 (keytab.hip): frame_mod tables built on the device, one workgroup per key (reference wmadd.cc:86-162, wmcommon.cc:143-202,
 * random.cc:97-161).  round_keys: 176 bytes per key (the AES-128 key schedule as FIPS-197's byte string, host/aes128.cc); sbox: the
 * 256 byte S-box; coded: the payload's convolutional code, 858 bytes (0 / 1) for an A block followed by 858 for a B block;
 * scratch: scratch_slots * key_table_scratch_bytes() bytes (n_keys <= scratch_slots: a launch's keys work side by side);
 * tables: n_keys * key_table_bytes() bytes, [2 (A, B)][2226 frames][81 bands] int8 KEEP 0 / UP 1 / DOWN 2. */
struct KeyTableArgs
{
  const unsigned char *round_keys;
  const unsigned char *sbox;
  const unsigned char *coded;
  unsigned char       *scratch;
  int                  scratch_slots;
  signed char         *tables;
  long long            n_keys;
};
size_t key_table_scratch_bytes();
size_t key_table_bytes();
hipError_t launch_frame_mod_tables (hipStream_t st, const KeyTableArgs& a);

/* K16t (keytab.hip): the TEMPLATES of many keys in one launch, one workgroup per key with K16's draws and shuffles: key i of the launch
 * writes tmpl + i * stride, stride entries of int16 in the format of host/wmcommon.cc build_frame_mod_template ([2 (A, B)][2226][81], zeros
 * behind the last one) -- what K16p reads.  tmpl is 16-byte aligned, stride a multiple of 16 of at least key_table_bytes() entries
 * (payload_table_stride (2226)).  KeyTableArgs::coded and ::tables are not used.  The default geometry only, like K16: mix on, two
 * frames per bit, 858 coded bits. */
struct KeyTemplateOut
{
  short    *tmpl;
  long long stride;
};
hipError_t launch_key_templates (hipStream_t st, const KeyTableArgs& a, const KeyTemplateOut& t);

/* K16p (keytab.hip): the frame_mod tables of MANY PAYLOADS with one key, expanded from the key's template (host/wmcommon.cc
 * build_frame_mod_template: int16 per (block type, frame, band): 0 / 1 / 2 as they are, 4 + 2 k + s = UP if coded bit k of the block type
 * xor s, else DOWN) in one launch: blockIdx.y = payload.  coded: n_payloads x [2 (A, B)][n_code] bytes 0 / 1; tables: n_payloads tables
 * of table_stride bytes each in K2's format, [2 * half_entries] int8 + padding.  table_stride is a multiple of 16 >= 2 * half_entries,
 * and the template holds table_stride entries (zeros behind the last one): every load and store is a whole 16-byte piece.
 * A template per table: tmpl_of (device, n_payloads ints) names the slot of table blockIdx.y, slot s begins at tmpl + s * tmpl_stride
 * (tmpl_stride: entries, a multiple of 8 >= table_stride); nullptr: every table reads tmpl itself.  The caller orders the tables by
 * slot, so that neighbouring workgroups share a template in L2. */
struct PayloadTableArgs
{
  const short         *tmpl;
  const int           *tmpl_of;
  long long            tmpl_stride;
  const unsigned char *coded;
  signed char         *tables;
  long long            table_stride;
  int                  half_entries;     // block_frames * 81: where the B block begins
  int                  n_code;
  int                  n_payloads;       // <= 65535
};
size_t     payload_table_stride (size_t block_frames);       // bytes between the tables of two payloads
hipError_t launch_payload_tables (hipStream_t st, const PayloadTableArgs& a);

/* K16g: the tables `get` needs for a clip with a key of its own (CLIP mode; reference syncfinder.cc:30-77 init_up_down, wmget.cc:52-108
 * mix_decode's entries, wmcommon.hh randomize_bit_order), from the same draws and shuffles as K16, one workgroup per key -- what the
 * host's build_clip_key_host produces (host/context.cc), table for table and byte for byte:
 *   chains      [key][12][170][8] u32   K5w: chain 2 bit + (0 up | 1 down), rows by frame: 30 band bytes + the next row's frame (u16)
 *   row_frames  [key][6][170] int       frame of every row (bit-major, by frame)
 *   want        [key][1020] int         the sync frames of the long block (two blocks), ascending
 *   perm        [key][1020] int         row w of the want list -> bit * 170 + row
 *   pos         [key][1020][81] u8      band -> 0 .. 29 (up), 30 .. 59 (down), 255 (not used) of want row w
 *   mix_frame   [key][51480] i16, mix_up / mix_down [key][51480] u8 (absolute band 20 .. 100): mix entry p
 *   inv_order   [key][858] int          inverse of the bit order permutation
 * KeyTableArgs::coded and ::tables are not used. */
struct ClipKeyTableOut
{
  unsigned int  *chains;
  int           *row_frames, *want, *perm;
  unsigned char *pos;
  short         *mix_frame;
  unsigned char *mix_up, *mix_down;
  int           *inv_order;
};
constexpr int CLIP_KEY_ROWS = 170, CLIP_KEY_WANT = 1020, CLIP_KEY_MIX = 51480, CLIP_KEY_CODED = 858;
hipError_t launch_clip_key_tables (hipStream_t st, const KeyTableArgs& a, const ClipKeyTableOut& out);

} // namespace awmk

namespace awmk {
/* I/O staging: interleaved PCM bytes <-> float32 on the device with the reference's
 * conversion rules (rawconverter.cc:155-286, rawconverter.hh:34-50).  width = bytes per value (1..4 integer, 4 / 8 float);
 * encoding 0 signed / 1 unsigned / 2 float; direct16 = the reference's native little-endian signed 16 bit rule
 * (truncate at 16 bit) instead of "clip to 32 bit, keep the top bits". */
struct PcmFormatDev { int width, encoding, big_endian, direct16; };
hipError_t launch_pcm_decode (hipStream_t st, const unsigned char *bytes, float *out, long long n_values, PcmFormatDev f);
hipError_t launch_pcm_encode (hipStream_t st, const float *in, unsigned char *bytes, long long n_values, PcmFormatDev f);

/* first / one-past-last non-zero value of an interleaved buffer (SyncFinder::scan_silence,
 * reference syncfinder.cc:155-169); result[0] = first (n_values if all zero), result[1] = last */
hipError_t launch_nonzero_range (hipStream_t st, const float *data, long long n_values, unsigned long long *result);

/* Stage 0 of a group of clips (ClipDecoder, reference wmget.cc:830-867, START position): the padded clips at 44.1 kHz side by side in one
 * buffer -- slice i = [pad_start_i zeros][clip i][pad zeros], slice_values each -- and the non-silent range of every slice (range[2 i] =
 * first non-zero value, absolute index in dst, -1 if there is none; range[2 i + 1] = last + 1).
 * Of the padding only `margin_values` on either side of a clip are written (the rest of a slice keeps whatever the buffer held): every
 * consumer of the slices skips the frames outside the non-silent range -- K4 / K4b per frame, K4s per row of fine offsets, K7 per item --
 * and the frames it does read reach at most 1024 + 8 * 64 frames (K4s: a row of 65 fine offsets, plus its read-ahead) beyond that range.
 * margin_values >= slice_values writes whole slices.
 * Every clip brings its descriptor: n_in frames at its own rate at `in` (nothing outside them is read), n44 frames at 44.1 kHz, pad_start,
 * and the geometry and table of its rate's fixed-ratio resampler (ctab / hl / np / step of the ResampleTable).  np == 0 marks a clip that
 * is at 44.1 kHz already (n_in == n44, no table): it is copied.  A resampled clip is K10 straight into its slice: output frame m of K10's
 * definition above, for the stream "hl - 1 null frames, the clip, null frames for ever", goes to pad_start + m C -- slice and range are bit
 * for bit those of launch_resample into a buffer and a copy from it, the products and sums come from K10's own tap code
 * (resample_slice_body / resample_phase_body), which reads its geometry from the descriptor: uniform per workgroup, scalar registers.
 * Three forms, one kernel each, each over its own clips only (grid.y):
 *   CLIP_FORM_GENERIC  the table and, for stereo with every resampled input of the group aligned, the tile's window in LDS (the generic taps
 *                      where the clip's table or window does not fit); dynamic LDS = the largest of the group
 *   CLIP_FORM_PHASE    the phase-per-thread form <147, 160, 18, 2, 8> for aligned stereo 48 kHz clips (awm_debug_set_resample_phase)
 *   CLIP_FORM_COPY     the 44.1 kHz clips
 * clip_stage_plan (host) chooses the form of every clip as launch_resample chooses for a stream of that rate, fills form / lds_floats /
 * in_span of src[0 .. n_clips) and writes list[0 .. n_clips): the slice indices form by form, in the order of the enum.  The launcher is
 * given the plan and the device copies of src and list; a form's workgroups find their slice in the form's part of the list -- or, where
 * every clip of the group has that form (a group at one rate), take blockIdx.y and load no list.  Launches per group:
 * clip_range_init_kernel and one per form PRESENT, whatever the number of clips or of distinct rates -- two for a group at one rate.
 * Tiles per workgroup: tiles of the group's longest clip x its clips / 4096, between 1 and 8.  Refused (hipErrorInvalidValue): dst not
 * 16-byte aligned, slice_values % 4, more than 65535 clips, more than 64 KiB of LDS, a plan made for the other input type.
 * Input types: launch_clip_stage reads float clips, launch_clip_stage_s16 SIGNED 16-BIT PCM (little-endian, interleaved: the reference's
 * native format, rawconverter.cc) with the plan made for it (s16 = true).  The descriptors are the same -- `in` holds the ADDRESS of the
 * clip's int16 values -- and slices and ranges are bit for bit what the float launcher writes for the decoded clips, float (v) * (1 /
 * 32768) (launch_pcm_decode): the same kernels instantiated for the other input type, whose loads convert and whose taps, sums, sinks,
 * zeros and ranges are the same code.  A value is converted once: on its way into the LDS window of the staged forms (the window stays
 * float2), or as the unstaged taps and the copy read it.
 * Alignment: a float clip may begin at any 4-byte address, an int16 clip at any EVEN address.  "Aligned" (stereo_aligned) means that a
 * stereo frame is one load -- every resampled input of the group 8-byte aligned (float) or 4-byte aligned (int16); a group with an input
 * that is not, or with another channel count, takes the generic taps with loads of one value.  The copy form loads single values. */
enum { CLIP_FORM_GENERIC = 0, CLIP_FORM_PHASE = 1, CLIP_FORM_COPY = 2 };
struct ClipStageSrc
{
  const float *in;
  long long    n_in, n44, pad_start;
  const float *ctab;                 // device, (np + 1) * hl; null for a copied clip
  int          hl, np, step;
  int          form;                 // CLIP_FORM_*
  int          lds_floats, in_span;  // CLIP_FORM_GENERIC: floats of the table in LDS (0: from global memory), frames of the tile's window (0: not staged)
};
struct ClipStagePlan
{
  int       n_channels = 0, n_clips = 0;
  int       n_form[3] = { 0, 0, 0 };
  long long max_n44 = 0;             // the group's longest clip: tiles per workgroup
  long long max_n44_form[3] = { 0, 0, 0 };
  bool      stereo_aligned = false;  // stereo and every resampled input 8-byte aligned (s16: 4-byte aligned)
  size_t    lds_bytes = 0;           // CLIP_FORM_GENERIC: the largest table + window of the group
  bool      s16 = false;             // the plan of launch_clip_stage_s16
};
ClipStagePlan clip_stage_plan (ClipStageSrc *src /* host */, int n_clips, int n_channels, int *list /* host */, bool s16 = false);
hipError_t launch_clip_stage (hipStream_t st, const ClipStagePlan& plan, const ClipStageSrc *src /* device */, const int *list /* device */,
                              float *dst, long long slice_values, long long margin_values, long long *range);
hipError_t launch_clip_stage_s16 (hipStream_t st, const ClipStagePlan& plan, const ClipStageSrc *src /* device */, const int *list /* device */,
                                  float *dst, long long slice_values, long long margin_values, long long *range);
}

namespace awmk {
/* ---- speed detection (reference wmspeed.cc; speed.hip) -------------------------------------------------------------- */
/* one centre speed of a scan pass, or the one ratio of a plain resample_ratio call: zita VResampler geometry */
struct SpeedCenterDev
{
  const float       *ctab;         // (256 + 1) rows of `stride` floats, hl coefficients each
  int                hl;           // taps per side
  int                stride;       // hl | 1 (odd: LDS bank spread)
  int                shift;        // input window of output m starts at (m * mant) >> shift
  unsigned long long mant;         // 53 bit mantissa of the phase step 256 / ratio
  double             frac_scale;   // fraction of that product -> phase 0 .. 256
  long long          n_in;         // input frames (after truncation)
  long long          n_out;        // output frames
  int                rows;         // K13 / K14: STFT rows of the half-rate clip
};
/* batch forms of K12 - K14 (..._batch_kernel): an entry of the launch is a (clip, centre) pair; entry e has centers[e] (n_in, n_out and rows
 * of its clip) and entries[e]: what the one-clip launch holds once in its arguments */
struct SpeedEntryDev
{
  const float         *in;           // K12: the clip
  const unsigned int  *cols;         // K13: column table of the clip's key
  const int           *col_frame;    // K14
  const unsigned char *col_first;    // K14
};
/* K12: VResampler (resample.cc:96-125); blockIdx.y = centre, outputs at out + centre * out_stride */
struct VarResampleArgs
{
  const float          *in;
  int                   n_channels;
  const SpeedCenterDev *centers;
  float                *out;
  long long             out_stride;    // floats
  int                   max_stride;    // largest table row stride among the centres (sizes the LDS copy)
  double                max_step;      // largest advance of the input window per output among the centres, in frames (mant / 2^shift); 0: unknown
  int                   lds_floats;    // set by the launcher
};
/* entries != nullptr: the batch form (a.in unused); entries_aligned: every clip of the launch is on an 8 byte address */
hipError_t launch_resample_var (hipStream_t st, const VarResampleArgs& a, long long max_n_out, int n_centers,
                                const SpeedEntryDev *entries = nullptr, bool entries_aligned = false);

/* K13: SpeedSync::prepare_mags (wmspeed.cc:204-268) */
struct SpeedMagsArgs
{
  const float          *sub;           // half-rate clips, [centre][sub_stride]
  long long             sub_stride;
  int                   n_channels;
  const SpeedCenterDev *centers;
  const float          *window512;     // FFTAnalyzer::gen_normalized_window (512)
  const unsigned int   *cols;          // [510][16] words: 30 up + 30 down band indices (0..80) per sync frame, columns [bit][frame asc]
  float2               *mags;          // [centre][510][ld] (umag, dmag)
  long long             mags_center_stride, ld;
};
hipError_t launch_speed_mags (hipStream_t st, const DevTables& t, const SpeedMagsArgs& a, int max_rows, int n_centers,
                              const SpeedEntryDev *entries = nullptr /* batch form: a.cols unused */);

/* K14: SpeedSync::compare (wmspeed.cc:270-395) */
struct SpeedItemDev { int center; double rel_speed_inv, q16_scale; };
struct SpeedCompareArgs
{
  const float2         *mags;
  long long             mags_center_stride, ld;
  const SpeedCenterDev *centers;
  const SpeedItemDev   *items;         // [n_centers][items_per_center]
  int                   n_centers, items_per_center;
  const int            *col_frame;     // [510] frame of the column
  const unsigned char  *col_first;     // [6][frames_per_block + 2]: columns of the bit with frame < f
  int                   frames_per_block, steps_per_frame, pad_start, rows_per_bit;
  double                min_delta;
  unsigned long long   *best;          // [items] bits of the best quality (zero initialised)
  int                   fold_groups = 0, n_ranges = 0;   // set by the launcher: groups of speeds folded into blockIdx.x (see launch_speed_compare)
};
hipError_t launch_speed_compare (hipStream_t st, const SpeedCompareArgs& a, int n_items,
                                 const SpeedEntryDev *entries = nullptr /* batch form: a.col_frame, a.col_first unused */);

/* K15 */
constexpr int ENERGY_PARTS = 256;
hipError_t launch_gather_values (hipStream_t st, const float *in, const unsigned long long *pos, long long n, float *out);
hipError_t launch_energy (hipStream_t st, const float *in, const long long *range /* [n][2] value index begin, end */, int n_ranges,
                          double *out /* [n][ENERGY_PARTS] */);
/* batch forms: positions / values of clip c at [first, first + n) of pos / out; a range carries its clip's base pointer */
struct GatherClipDev  { const float *in; long long first, n; };
struct EnergyRangeDev { const float *in; long long begin, end; };
hipError_t launch_gather_values_batch (hipStream_t st, const GatherClipDev *clips, int n_clips, long long max_n, const unsigned long long *pos, float *out);
hipError_t launch_energy_batch (hipStream_t st, const EnergyRangeDev *range, int n_ranges, double *out /* [n][ENERGY_PARTS] */);
}
