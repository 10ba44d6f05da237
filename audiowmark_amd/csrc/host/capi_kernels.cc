// C ABI: kernel-level and pipeline-level entry points -- see include/awm_hip.h
#include "context.hh"
#include "syncfinder.hh"
#include "wmget.hh"
#include "wmdecode.hh"
#include "wmspeed.hh"
#include "utils.hh"
#include "wmfile.hh"
#include "keytab_stage.hh"
#include <sys/stat.h>
#include <atomic>
#include <future>
#include <thread>
#include <tuple>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace awm;
namespace awm { Key capi_key (const uint8_t key[16]); }
namespace awm { extern int g_key_tables_on_device; int clip_key_tables_check (awm_ctx *ctx, const uint8_t *keys, size_t n_keys, long long mismatch_out[9]); }       // wmget.cc (also read by the clip batches of `get`)

namespace {

constexpr int LIMITER_BLOCK = Params::mark_sample_rate * int (Params::limiter_block_size_ms) / 1000;   // Limiter::set_block_size_ms
const float LIMITER_CEILING = float (Params::limiter_ceiling);

constexpr int MAX_FRAMES_PER_BIT = 8;

int
check_ctx (awm_ctx *ctx)
{
  if (!ctx)
    {
      set_error ("null context");
      return AWM_ERR_ARG;
    }
  hipError_t e = hipSetDevice (ctx->device);
  if (e != hipSuccess)
    {
      set_error ("hipSetDevice: " + hip_error_string (e));
      return AWM_ERR_HIP;
    }
  if (params().frames_per_bit < 1 || params().frames_per_bit > MAX_FRAMES_PER_BIT || params().payload_size != 128)
    {
      // --frames-per-bit (audiowmark.cc:675-679) sets the block's geometry -- 510 sync + 858 x frames_per_bit data frames --, which every
      // kernel takes as an argument; the tables that are BUILT on the device (K16 / K16g: clip batches with a key per clip) are laid
      // out for the default and hand over to the host builders otherwise.  The deprecated --short payloads are out of scope.
      set_error ("unsupported watermark parameters (frames_per_bit outside 1 .. 8 or a short payload)");
      return AWM_ERR_ARG;
    }
  return 0;
}

// prologue of every entry point that takes a context: the context's own settings (if it has any) are in force for the calling
// thread until the entry point returns, the device is selected, unsupported block geometries are refused
#define AWM_ENTER(ctx) \
  awm::ParamsBind params_bind__ ((ctx) ? (ctx)->own_params.get() : nullptr); \
  if (int rc__ = check_ctx (ctx)) return rc__

int
frames_per_span (awm_ctx *ctx, long long n_frames1024, int waves_per_simd = 0)       // 0: the fused add kernel's (K2) own occupancy
{
  // Every wave streams through L frames plus 2 halo frames.  All waves of one "round" (CUs x resident waves) start
  // and finish together, so pick the number of rounds k that minimises k * (L + 2) with L = ceil (F / (k * capacity)):
  // long spans amortise the halo, whole rounds avoid a half-empty tail.
  static int cus = 0;
  if (!cus)
    {
      hipDeviceProp_t prop;
      cus = 256;
      if (hipGetDeviceProperties (&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0)
        cus = prop.multiProcessorCount;
    }
  const int capacity = cus * 4 * (waves_per_simd > 0 ? waves_per_simd : awmk::add_mix_waves_per_simd());       // resident waves of the fused add kernel
  long long best_l = 4, best_cost = -1;
  for (int k = 1; k <= 16; k++)
    {
      long long l = (n_frames1024 + (long long) k * capacity - 1) / ((long long) k * capacity);
      l = std::max<long long> (l, 4);
      const long long cost = k * (l + 2);
      if (best_cost < 0 || cost < best_cost)
        {
          best_cost = cost;
          best_l = l;
        }
    }
  return int (std::min<long long> (best_l, 4096));
}

// the fields of K2's (AddMixArgs) and K2m's (AddMixMultiArgs) arguments that depend on no stream, span or payload
template<class Args> void
fill_add_mix_common (Args& a, double water_delta)
{
  // powf (mag, -params().water_delta * data_bit_sign): double product converted to float (reference wmadd.cc:79)
  a.neg_delta_up = float (-water_delta * 1);
  a.neg_delta_down = float (-water_delta * -1);
  a.limiter_block = LIMITER_BLOCK;
  a.block_frames = int (mark_block_frame_count());
  a.frames_pad_start = int (Params::frames_pad_start);
}

/* K2m over n_payloads outputs: passes of at most ADD_MULTI_TILE outputs and of nearly equal size (5 payloads: 3 + 2, not 4 + 1: a pass costs the
 * input read and the forward transforms whatever it carries).  output (p, o) fills in output p (false: give up; the tables of a pass are looked
 * up when it is launched), launch() enqueues the pass that a describes, after (p0, n) what follows the pass of outputs p0 .. p0 + n - 1 */
template<class Output, class Launch, class After> int
add_mix_multi_passes (awm_ctx *ctx, hipStream_t st, awmk::AddMixMultiArgs& a, size_t n_payloads, Output&& output, Launch&& launch, After&& after)
{
  const size_t n_passes = (n_payloads + awmk::ADD_MULTI_TILE - 1) / awmk::ADD_MULTI_TILE;
  size_t p0 = 0;
  for (size_t pass = 0; pass < n_passes; pass++)
    {
      const size_t n = n_payloads / n_passes + (pass < n_payloads % n_passes ? 1 : 0);
      for (size_t i = 0; i < size_t (awmk::ADD_MULTI_TILE); i++)
        {
          a.o[i] = awmk::AddMixOut {};
          if (i < n && !output (p0 + i, a.o[i]))
            return AWM_ERR_ARG;
        }
      a.n_out = int (n);
      {
        ProfScope ps (ctx, PROF_ADD_MIX_MULTI, double (1 + n) * double (a.n_frames) * a.n_channels * 4.0, st);     // the input once, every output once
        if (int rc = launch())
          return rc;
      }
      if (int rc = after (p0, n))
        return rc;
      p0 += n;
    }
  return 0;
}

void
fill_pattern (const ResultSet::Pattern& p, awm_pattern& o)
{
  o.time = p.time;
  o.sync_index = p.sync_score.index;
  o.sync_quality = p.sync_score.quality;
  o.block_type = int (p.sync_score.block_type);
  o.type = int (p.type);
  o.decode_error = p.decode_error;
  o.speed = p.speed;
  o.n_bits = std::min<int> (p.bit_vec.size(), 128);
  for (int b = 0; b < o.n_bits; b++)
    o.bits[b] = p.bit_vec[b];
}

// the results of a batch of clips: clip i's patterns to out[i * max_out_per_clip ...], their number (possibly more) to n_out[i]
void
fill_batch_patterns (const std::vector<ResultSet>& sets, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  for (size_t i = 0; i < sets.size(); i++)
    {
      n_out[i] = int (sets[i].patterns.size());
      for (size_t j = 0; j < sets[i].patterns.size() && j < max_out_per_clip; j++)
        fill_pattern (sets[i].patterns[j], out[i * max_out_per_clip + j]);
    }
}

DeviceWav
make_wav (const float *pcm_d, size_t n_frames, int n_channels)
{
  DeviceWav w;
  w.data = pcm_d;
  w.n_frames = n_frames;
  w.n_channels = n_channels;
  w.sample_rate = Params::mark_sample_rate;
  return w;
}

DeviceWav
make_wav_rate (const float *pcm_d, size_t n_frames, int n_channels, int rate)
{
  DeviceWav w = make_wav (pcm_d, n_frames, n_channels);
  w.sample_rate = rate;
  return w;
}

} // namespace

extern "C" {

int
awm_stft_d (awm_ctx *ctx, const float *pcm_d, size_t n_frames, int n_channels, size_t start_index, size_t hop,
            size_t frame_count, float *out_d)
{
  AWM_ENTER (ctx);
  if (!pcm_d || !out_d || n_channels < 1)
    {
      set_error ("awm_stft_d: bad argument");
      return AWM_ERR_ARG;
    }
  if (frame_count && n_frames < start_index + (frame_count - 1) * hop + Params::frame_size)
    {
      set_error ("awm_stft_d: range exceeds the data");
      return AWM_ERR_ARG;
    }
  ProfScope ps (ctx, PROF_STFT, double (frame_count) * n_channels * 8200.0);
  AWM_HIP_CHECK (awmk::launch_stft_full (ctx->stream, ctx->tabs, pcm_d, n_channels, (long long) start_index, (long long) hop,
                                         (long long) frame_count, reinterpret_cast<float2 *> (out_d)));
  return 0;
}

int
awm_add_init_block_max_d (awm_ctx *ctx, float *block_max_d, size_t n_blocks)
{
  AWM_ENTER (ctx);
  unsigned int bits;
  std::memcpy (&bits, &LIMITER_CEILING, sizeof (bits));
  AWM_HIP_CHECK (awmk::launch_fill_u32 (ctx->stream, reinterpret_cast<unsigned int *> (block_max_d), bits, n_blocks));
  return 0;
}

static int
add_mix_impl (awm_ctx *ctx, const float *pcm_in_d, float *out_d, size_t n_frames, int n_channels,
              const int8_t *frame_mod_dev, double water_delta, size_t first_frame,
              const float *halo_before_d, const float *halo_after_d, float *block_max_d, size_t first_block, size_t n_blocks,
              WorkLane *lane = nullptr, int delta_only = 0, bool s16 = false)
{
  // (s16: pcm_in_d and the halos hold the addresses of int16 values, K2 instantiated for 16-bit input; counted under the float K2's scope)
  hipStream_t st = lane ? lane->stream : ctx->stream;
  awmk::AddMixArgs a {};
  a.pcm_in = pcm_in_d;
  a.out = out_d;
  a.n_frames = (long long) n_frames;
  a.n_channels = n_channels;
  a.frame_mod = frame_mod_dev;
  fill_add_mix_common (a, water_delta);
  a.first_frame = (long long) first_frame;
  a.halo_before = halo_before_d;
  a.halo_after = halo_after_d;
  a.block_max = reinterpret_cast<unsigned int *> (block_max_d);
  a.first_block = (long long) first_block;
  a.n_blocks = (long long) n_blocks;
  a.frames_per_span = frames_per_span (ctx, (long long) (n_frames + 1023) / 1024);
  a.delta_only = delta_only;
  {
    ProfScope ps (ctx, PROF_ADD_MIX, double (n_frames) * n_channels * (s16 ? 6.0 : 8.0), st);     // read + write every sample once
    AWM_HIP_CHECK (s16 ? awmk::launch_add_mix_s16 (st, ctx->tabs, a) : awmk::launch_add_mix (st, ctx->tabs, a));
  }
  if (ctx->snr_on && s16)
    AWM_HIP_CHECK (awmk::launch_power_sums_s16 (st, reinterpret_cast<const int16_t *> (pcm_in_d), out_d, (long long) (n_frames * n_channels),
                                                ctx->ws_snr.as<double>()));
  else if (ctx->snr_on)               // add --snr: the mix before the limiter (reference wmadd.cc:553-563)
    AWM_HIP_CHECK (awmk::launch_power_sums (st, pcm_in_d, out_d, (long long) (n_frames * n_channels), ctx->ws_snr.as<double>()));
  return 0;
}

} // extern "C"
namespace awm {
int
add_mix_device (awm_ctx *ctx, const float *pcm_in_d, float *out_d, size_t n_frames, int n_channels, const int8_t *frame_mod_dev,
                double water_delta, size_t first_frame, const float *halo_before_d, const float *halo_after_d, float *block_max_d,
                size_t first_block, size_t n_blocks)
{
  return add_mix_impl (ctx, pcm_in_d, out_d, n_frames, n_channels, frame_mod_dev, water_delta, first_frame, halo_before_d, halo_after_d,
                       block_max_d, first_block, n_blocks);
}
}
extern "C" {

int
awm_ctx_snr_begin (awm_ctx *ctx)
{
  AWM_ENTER (ctx);
  if (int rc = ctx->ws_snr.reserve (2 * sizeof (double))) return rc;
  AWM_HIP_CHECK (hipMemsetAsync (ctx->ws_snr.ptr, 0, 2 * sizeof (double), ctx->stream));
  AWM_HIP_CHECK (hipStreamSynchronize (ctx->stream));          // (the lanes' streams start after this)
  ctx->snr_on = true;
  return 0;
}

int
awm_ctx_snr_end (awm_ctx *ctx, double *signal_power, double *delta_power)
{
  AWM_ENTER (ctx);
  if (!ctx->snr_on)
    {
      set_error ("awm_ctx_snr_end without awm_ctx_snr_begin");
      return AWM_ERR_ARG;
    }
  ctx->snr_on = false;
  double acc[2] = { 0, 0 };
  AWM_HIP_CHECK (hipDeviceSynchronize());
  AWM_HIP_CHECK (hipMemcpy (acc, ctx->ws_snr.ptr, sizeof (acc), hipMemcpyDeviceToHost));
  if (delta_power)
    *delta_power = acc[0];
  if (signal_power)
    *signal_power = acc[1];
  return 0;
}

int
awm_add_mix_d (awm_ctx *ctx, const float *pcm_in_d, float *out_d, size_t n_frames, int n_channels,
               const int8_t *frame_mod, double water_delta, size_t first_frame,
               const float *halo_before_d, const float *halo_after_d,
               float *block_max_d, size_t first_block, size_t n_blocks)
{
  AWM_ENTER (ctx);
  if (!pcm_in_d || !out_d || !frame_mod || n_channels < 1)
    {
      set_error ("awm_add_mix_d: bad argument");
      return AWM_ERR_ARG;
    }
  const size_t table_bytes = 2 * mark_block_frame_count() * Params::n_bands;
  if (int rc = ctx->ws_misc.reserve (table_bytes)) return rc;
  AWM_HIP_CHECK (hipMemcpyAsync (ctx->ws_misc.ptr, frame_mod, table_bytes, hipMemcpyHostToDevice, ctx->stream));
  return add_mix_impl (ctx, pcm_in_d, out_d, n_frames, n_channels, ctx->ws_misc.as<int8_t>(), water_delta, first_frame,
                       halo_before_d, halo_after_d, block_max_d, first_block, n_blocks);
}

int
awm_add_limit_d (awm_ctx *ctx, float *out_d, size_t n_frames, int n_channels, size_t first_sample,
                 const float *block_max_d, size_t first_block, size_t n_blocks)
{
  AWM_ENTER (ctx);
  const size_t tab_entries = awmk::limiter_tab_entries ((long long) n_frames, (long long) first_sample, LIMITER_BLOCK);
  if (int rc = ctx->ws_limit_tab.reserve ((tab_entries + 1) * sizeof (float2))) return rc;
  ProfScope ps (ctx, PROF_LIMITER, double (n_frames) * n_channels * 8.0);
  AWM_HIP_CHECK (awmk::launch_limiter (ctx->stream, out_d, (long long) n_frames, n_channels, (long long) first_sample, block_max_d,
                                       (long long) first_block, (long long) n_blocks, LIMITER_BLOCK, LIMITER_CEILING,
                                       ctx->ws_limit_tab.as<float2>(), tab_entries));
  return 0;
}

/* The two halves on signed 16-bit PCM (include/awm_hip.h): K2 instantiated for 16-bit input, and the last pass -- ramp, encode, store -- of
 * a whole stream.  Refusals before anything is enqueued. */
int
awm_add_mix_s16_d (awm_ctx *ctx, const int16_t *pcm_in_d, float *out_d, size_t n_frames, int n_channels,
                   const int8_t *frame_mod, double water_delta, size_t first_frame,
                   const int16_t *halo_before_d, const int16_t *halo_after_d,
                   float *block_max_d, size_t first_block, size_t n_blocks)
{
  AWM_ENTER (ctx);
  const char *bad = nullptr;
  if (n_channels < 1)
    bad = "n_channels < 1";
  else if ((reinterpret_cast<uintptr_t> (pcm_in_d) | reinterpret_cast<uintptr_t> (halo_before_d) | reinterpret_cast<uintptr_t> (halo_after_d)) & 1)
    bad = "an int16 pointer is not 2-byte aligned";
  else if (!frame_mod || (n_frames && (!pcm_in_d || !out_d)))
    bad = "null pointer";
  if (bad)
    {
      set_error (std::string ("awm_add_mix_s16_d: ") + bad);
      return AWM_ERR_ARG;
    }
  if (!n_frames)
    return 0;
  const size_t table_bytes = 2 * mark_block_frame_count() * Params::n_bands;
  if (int rc = ctx->ws_misc.reserve (table_bytes)) return rc;
  AWM_HIP_CHECK (hipMemcpyAsync (ctx->ws_misc.ptr, frame_mod, table_bytes, hipMemcpyHostToDevice, ctx->stream));
  return add_mix_impl (ctx, reinterpret_cast<const float *> (pcm_in_d), out_d, n_frames, n_channels, ctx->ws_misc.as<int8_t>(), water_delta, first_frame,
                       reinterpret_cast<const float *> (halo_before_d), reinterpret_cast<const float *> (halo_after_d), block_max_d, first_block,
                       n_blocks, nullptr, 0, /* s16 */ true);
}

/* one pass of the last pass on a lane: the table entries of its own blocks, then ramp + encode + store (counted under limit_encode_s16_kernel) */
static int
limit_encode_pass (awm_ctx *ctx, WorkLane *lane, const float *mix_d, int16_t *out_d, size_t n_frames, int n_channels, size_t first_sample,
                   const float *block_max_d, size_t first_block, size_t n_blocks, int limiter_block, const int16_t *orig_d = nullptr)
{
  float2 *tab = nullptr;
  size_t tab_entries = 0;
  if (block_max_d)
    {
      tab_entries = awmk::limiter_tab_entries ((long long) n_frames, (long long) first_sample, limiter_block);
      if (int rc = lane->ws_limit_tab.reserve ((tab_entries + 1) * sizeof (float2))) return rc;
      tab = lane->ws_limit_tab.as<float2>();
    }
  ProfScope ps (ctx, PROF_LIMIT_ENCODE_S16, double (n_frames) * n_channels * (orig_d ? 8.0 : 6.0), lane->stream);
  AWM_HIP_CHECK (awmk::launch_limit_encode (lane->stream, mix_d, out_d, (long long) n_frames, n_channels, (long long) first_sample, block_max_d,
                                            (long long) first_block, (long long) n_blocks, limiter_block, LIMITER_CEILING, tab, tab_entries, orig_d));
  return 0;
}

int
awm_add_limit_s16_d (awm_ctx *ctx, const float *mix_d, int16_t *out_d, size_t n_frames, int n_channels, size_t first_sample,
                     const float *block_max_d, size_t first_block, size_t n_blocks)
{
  AWM_ENTER (ctx);
  const char *bad = nullptr;
  if (n_channels < 1)
    bad = "n_channels < 1";
  else if (reinterpret_cast<uintptr_t> (out_d) & 1)
    bad = "out_d is not 2-byte aligned";
  else if (n_frames && (!mix_d || !out_d))
    bad = "null pointer";
  if (bad)
    {
      set_error (std::string ("awm_add_limit_s16_d: ") + bad);
      return AWM_ERR_ARG;
    }
  if (!n_frames)
    return 0;
  return limit_encode_pass (ctx, ctx, mix_d, out_d, n_frames, n_channels, first_sample, block_max_d, first_block, n_blocks, LIMITER_BLOCK);
}

/* (measurement knob, tools/gpu_add_slabs.py) `add` in slabs of this many MB of output: the fused add of slab s, then the limiter for
 * everything whose look-ahead second is complete -- so that the limiter re-reads what the add has just written while it may still
 * be in the 256 MB memory-side cache.  0 (default): one add over the whole stream, then one limiter pass.  DESIGN.md section 3 has
 * the sweep: the fused add needs 4096 resident waves x long spans (the 2 halo frames per span are its overhead), a slab small enough
 * for the cache starves it. */
static int g_add_slab_mb = 0;
extern "C" void awm_debug_set_add_slab_mb (int mb) { g_add_slab_mb = mb < 0 ? 0 : mb; }

/* `add` reads three frames of the input per frame of the output (the overlap-add of the neighbours' watermark signal): an output that
 * overlaps the input anywhere is a race between workgroups.  The entry points that take both pointers from the caller refuse it before
 * anything is enqueued. */
static bool
add_buffers_overlap (const float *in, const float *out, size_t n_values)
{
  const uintptr_t a = reinterpret_cast<uintptr_t> (in), b = reinterpret_cast<uintptr_t> (out), bytes = n_values * sizeof (float);
  return a < b + bytes && b < a + bytes;
}

/* where the passes of the last stage of a whole-stream `add` end: with marks (awm_add_get_watermark_d and its 16-bit twin) one pass per
 * range of `get`'s chunk ends, rounded up to whole limiter blocks, else one pass */
static std::vector<size_t>
last_pass_ends (size_t n_frames, int n_channels, bool per_chunk)
{
  std::vector<size_t> ends;
  if (per_chunk)
    for (const ChunkRange& c : plan_chunks (n_frames, n_channels))
      {
        size_t e = std::min (n_frames, (c.first_frame + c.n_frames + LIMITER_BLOCK - 1) / LIMITER_BLOCK * size_t (LIMITER_BLOCK));
        if (e < n_frames && n_frames - e < size_t (LIMITER_BLOCK))          // (no sliver of a last pass)
          e = n_frames;
        if (ends.empty() || e > ends.back())
          ends.push_back (e);
      }
  if (ends.empty() || ends.back() != n_frames)
    ends.push_back (n_frames);
  return ends;
}

/* add_full from and to 16-bit PCM (awm_add_watermark_s16_d at 44.1 kHz), every channel count and any even address: K2 reads the int16
 * values and writes the un-limited float mix into the lane's grow-only workspace, the last pass -- ramp, encode, store -- runs per range
 * and leaves an event behind each when marks are armed.  out_d may be pcm_in_d: K2 has consumed the input before the first pass stores.
 * No decode and no encode launch; the slab switch of add_full does not apply. */
static int
add_full_s16 (awm_ctx *ctx, const int16_t *pcm_in_d, int16_t *out_d, size_t n_frames, int n_channels,
              const int8_t *frame_mod_dev, double water_delta, int use_limiter, WorkLane *lane = nullptr, ReadyMarks *marks = nullptr)
{
  if (!lane)
    lane = ctx;
  if (marks)
    {
      marks->disarm();
      marks->base = out_d;
      marks->n_frames = n_frames;
    }
  hipStream_t st = lane->stream;
  float *block_max = nullptr;
  const size_t n_blocks = n_frames / LIMITER_BLOCK + 2;
  if (use_limiter)
    {
      if (int rc = lane->ws_block_max.reserve (n_blocks * sizeof (float))) return rc;
      block_max = lane->ws_block_max.as<float>();
      unsigned int bits;
      std::memcpy (&bits, &LIMITER_CEILING, sizeof (bits));
      AWM_HIP_CHECK (awmk::launch_fill_u32 (st, reinterpret_cast<unsigned int *> (block_max), bits, n_blocks));
    }
  if (int rc = lane->ws_add_mix.reserve (n_frames * n_channels * sizeof (float))) return rc;
  float *mix = lane->ws_add_mix.as<float>();
  if (int rc = add_mix_impl (ctx, reinterpret_cast<const float *> (pcm_in_d), mix, n_frames, n_channels, frame_mod_dev, water_delta, 0, nullptr, nullptr,
                             block_max, 0, n_blocks, lane, 0, /* s16 */ true))
    return rc;
  size_t done = 0;
  for (size_t e : last_pass_ends (n_frames, n_channels, marks != nullptr))
    {
      // (the passes share the lane's ramp table: they run in stream order, a pass rebuilds the entries of its own blocks)
      if (int rc = limit_encode_pass (ctx, lane, mix + done * n_channels, out_d + done * n_channels, e - done, n_channels, done, block_max, 0, n_blocks,
                                      LIMITER_BLOCK))
        return rc;
      done = e;
      if (marks)
        {
          hipEvent_t ev = marks->next_event();
          if (!ev)
            {
              set_error ("cannot create an event");
              return AWM_ERR_HIP;
            }
          AWM_HIP_CHECK (hipEventRecord (ev, st));
          marks->marks.push_back ({ e, ev });
        }
    }
  if (marks)
    marks->armed = true;
  return 0;
}

/* whole stream on one lane (stream + block maxima + limiter table of that lane; the context itself is lane 0) */
static int
add_full (awm_ctx *ctx, const float *pcm_in_d, float *out_d, size_t n_frames, int n_channels,
          const int8_t *frame_mod_dev, double water_delta, int use_limiter, WorkLane *lane = nullptr, ReadyMarks *marks = nullptr)
{
  if (!lane)
    lane = ctx;
  if (marks)
    {
      marks->disarm();
      marks->base = out_d;
      marks->n_frames = n_frames;
    }
  hipStream_t st = lane->stream;
  float *block_max = nullptr;
  const size_t n_blocks = n_frames / LIMITER_BLOCK + 2;
  if (use_limiter)
    {
      if (int rc = lane->ws_block_max.reserve (n_blocks * sizeof (float))) return rc;
      block_max = lane->ws_block_max.as<float>();
      unsigned int bits;
      std::memcpy (&bits, &LIMITER_CEILING, sizeof (bits));
      AWM_HIP_CHECK (awmk::launch_fill_u32 (st, reinterpret_cast<unsigned int *> (block_max), bits, n_blocks));
    }
  const size_t FRAME = Params::frame_size;
  size_t slab = g_add_slab_mb ? (size_t (g_add_slab_mb) << 20) / (n_channels * sizeof (float)) / FRAME * FRAME : 0;    // sample frames
  if (!use_limiter || pcm_in_d == out_d || slab < 64 * FRAME || n_frames < 2 * slab)
    slab = 0;
  if (slab)
    {
      // slabs of whole 1024-sample frames, the last one takes the rest; each one is a span with its neighbours' frames as halos
      // (add_mix_impl: the same entry the multi-GPU spans use -- output bit-identical to the whole-stream launch)
      const size_t tab_entries = awmk::limiter_tab_entries ((long long) n_frames, 0, LIMITER_BLOCK);
      if (int rc = lane->ws_limit_tab.reserve ((tab_entries + 1) * sizeof (float2))) return rc;
      const size_t n_slabs = n_frames / slab;
      size_t limited = 0;                                  // the limiter has run for samples [0, limited)
      for (size_t i = 0; i < n_slabs; i++)
        {
          const size_t a = i * slab, b = i + 1 == n_slabs ? n_frames : a + slab;
          if (int rc = add_mix_impl (ctx, pcm_in_d + a * n_channels, out_d + a * n_channels, b - a, n_channels, frame_mod_dev, water_delta,
                                     a / FRAME, a ? pcm_in_d + (a - FRAME) * n_channels : nullptr, b < n_frames ? pcm_in_d + b * n_channels : nullptr,
                                     block_max, 0, n_blocks, lane))
            return rc;
          // the ramp of limiter block k needs the maxima of k - 1, k, k + 1 (limiter.cc:99-124): complete once the add has passed (k + 2) BS
          const size_t upto = b == n_frames ? n_frames : (b / LIMITER_BLOCK >= 1 ? (b / LIMITER_BLOCK - 1) * size_t (LIMITER_BLOCK) : 0);
          if (upto > limited)
            {
              ProfScope ps (ctx, PROF_LIMITER, double (upto - limited) * n_channels * 8.0, st);
              // (the passes share the lane's ramp table: they run in stream order, a pass rebuilds the entries of its own blocks)
              AWM_HIP_CHECK (awmk::launch_limiter (st, out_d + limited * n_channels, (long long) (upto - limited), n_channels, (long long) limited, block_max, 0,
                                                   (long long) n_blocks, LIMITER_BLOCK, LIMITER_CEILING, lane->ws_limit_tab.as<float2>(), tab_entries));
              limited = upto;
            }
        }
      return 0;
    }
  if (int rc = add_mix_impl (ctx, pcm_in_d, out_d, n_frames, n_channels, frame_mod_dev, water_delta, 0, nullptr, nullptr,
                             block_max, 0, n_blocks, lane))
    return rc;
  // With marks (awm_add_get_watermark_d) the limiter runs in one pass per range of `get`'s chunk ends (every block maximum is known
  // after the mix: a pass needs nothing from the passes after it) and leaves an event behind each: the chunk that ends there may start.
  const std::vector<size_t> ends = last_pass_ends (n_frames, n_channels, marks != nullptr);
  if (use_limiter)
    {
      const size_t tab_entries = awmk::limiter_tab_entries ((long long) n_frames, 0, LIMITER_BLOCK);
      if (int rc = lane->ws_limit_tab.reserve ((tab_entries + 1) * sizeof (float2))) return rc;
      size_t limited = 0;
      for (size_t e : ends)
        {
          {
            ProfScope ps (ctx, PROF_LIMITER, double (e - limited) * n_channels * 8.0, st);
            // (the passes share the lane's ramp table: they run in stream order, a pass rebuilds the entries of its own blocks)
            AWM_HIP_CHECK (awmk::launch_limiter (st, out_d + limited * n_channels, (long long) (e - limited), n_channels, (long long) limited, block_max, 0,
                                                 (long long) n_blocks, LIMITER_BLOCK, LIMITER_CEILING, lane->ws_limit_tab.as<float2>(), tab_entries));
          }
          limited = e;
          if (marks)
            {
              hipEvent_t ev = marks->next_event();
              if (!ev)
                {
                  set_error ("cannot create an event");
                  return AWM_ERR_HIP;
                }
              AWM_HIP_CHECK (hipEventRecord (ev, st));
              marks->marks.push_back ({ e, ev });
            }
        }
    }
  else if (marks)
    {
      hipEvent_t ev = marks->next_event();
      if (!ev)
        {
          set_error ("cannot create an event");
          return AWM_ERR_HIP;
        }
      AWM_HIP_CHECK (hipEventRecord (ev, st));
      marks->marks.push_back ({ n_frames, ev });
    }
  if (marks)
    marks->armed = true;
  return 0;
}

/* ResamplerImpl::create (reference resample.cc:233-270): zita's fixed-ratio Resampler if it takes the two rates, else
 * its VResampler with ratio new / old.  Both run as closed forms of the streaming classes (K10 / K12). */
struct RateConverter
{
  const ResampleTable *fixed = nullptr;
  VarResampleGeometry  var;
  double               ratio = 0;
  bool ok() const { return fixed || var.ok; }
  int  hl() const { return fixed ? fixed->hl : var.hl; }
  // input frame (of the stream without the leading null frames) where the window of output m starts + hl - 1
  size_t window_start (size_t m) const
  {
    return fixed ? size_t ((static_cast<unsigned __int128> (m) * unsigned (fixed->step)) / unsigned (fixed->np)) : var.window_start (m);
  }
  /* frames the streaming resampler delivers for n_in input frames when it is fed "hl - 1 null frames, the input, hl null
   * frames" (WavChunkLoader at EOF, wavchunkloader.cc:200-216): every m with window_start (m) <= n_in - 1 */
  size_t stream_frames (size_t n_in) const
  {
    if (fixed)
      return resample_fixed_frames (*fixed, n_in);
    return var.stream_frames (n_in);
  }
};

static RateConverter
rate_converter (awm_ctx *ctx, int rate_in, int rate_out)
{
  RateConverter rc;
  if (rate_in <= 0 || rate_out <= 0)
    return rc;
  rc.fixed = ctx->get_resample_table (rate_in, rate_out);
  if (!rc.fixed)
    {
      rc.ratio = double (rate_out) / rate_in;
      rc.var = var_resample_geometry (rc.ratio);
      if (!rc.var.ok)
        set_error (string_printf ("resampling from old_rate=%d to new_rate=%d not implemented", rate_in, rate_out));
    }
  return rc;
}

static int
resample_device (awm_ctx *ctx, const RateConverter& conv, const float *in_d, size_t n_in, int n_channels, float *out_d, size_t n_out)
{
  if (!conv.fixed)
    return resample_var_device (ctx, ctx, in_d, n_in, n_channels, conv.ratio, out_d, n_out);
  const ResampleTable& t = *conv.fixed;
  awmk::ResampleArgs ra {};
  ra.in = in_d;
  ra.n_in = (long long) n_in;
  ra.n_channels = n_channels;
  ra.ctab = t.ctab.as<float>();
  ra.hl = t.hl;
  ra.np = t.np;
  ra.step = t.step;
  ra.out = out_d;
  ra.n_out = (long long) n_out;
  ProfScope ps (ctx, PROF_RESAMPLE, double (n_in + n_out) * n_channels * 4.0);      // every input and output sample once
  AWM_HIP_CHECK (awmk::launch_resample (ctx->stream, ra));
  return 0;
}

size_t
awm_resample_frames (awm_ctx *ctx, size_t n_frames, int rate_in, int rate_out)
{
  if (check_ctx (ctx))
    return 0;
  const RateConverter conv = rate_converter (ctx, rate_in, rate_out);
  return conv.ok() ? conv.stream_frames (n_frames) : 0;
}

int
awm_resample_d (awm_ctx *ctx, const float *pcm_in_d, size_t n_frames, int n_channels, int rate_in, int rate_out,
                float *out_d, size_t n_out_frames)
{
  AWM_ENTER (ctx);
  const RateConverter conv = rate_converter (ctx, rate_in, rate_out);
  if (!conv.ok())
    return AWM_ERR_ARG;
  if ((n_frames && !pcm_in_d) || (n_out_frames && !out_d) || n_channels < 1)
    {
      set_error ("awm_resample_d: bad argument");
      return AWM_ERR_ARG;
    }
  return resample_device (ctx, conv, pcm_in_d, n_frames, n_channels, out_d, n_out_frames);
}

/* add_stream_watermark for a stream at another rate (WatermarkResampler, reference wmadd.cc:353-430 + 520-589): the
 * input is resampled to 44.1 kHz, the watermark SIGNAL is generated there frame by frame, resampled back and added to
 * the original; limiter blocks are one second at the input rate.  The reference feeds zero frames after the input until
 * everything is written, so every stage simply sees a zero extended input here. */
static int
add_full_rate (awm_ctx *ctx, const float *pcm_in_d, float *out_d, size_t n_frames, int C, const int8_t *frame_mod_dev,
               double water_delta, int use_limiter, int rate)
{
  const RateConverter down = rate_converter (ctx, rate, Params::mark_sample_rate);
  const RateConverter up = rate_converter (ctx, Params::mark_sample_rate, rate);
  if (!down.ok() || !up.ok())
    return AWM_ERR_ARG;
  if (!n_frames)
    return 0;
  // watermark frames (44.1 kHz) the last output sample can reach: window of output n ends at floor (n s / np) + hl (input index)
  const size_t last44 = up.window_start (n_frames - 1) + size_t (up.hl()) + 1;
  const size_t F = last44 / Params::frame_size + 1;              // watermark frames 0 .. F - 1 are needed
  const size_t n44 = (F + 1) * Params::frame_size;               // frame F's delta completes frame F - 1
  if (int rc = ctx->ws_rate_a.reserve (n44 * C * sizeof (float))) return rc;
  if (int rc = ctx->ws_rate_b.reserve (n44 * C * sizeof (float))) return rc;
  if (int rc = ctx->ws_rate_c.reserve (n_frames * C * sizeof (float))) return rc;
  float *x44 = ctx->ws_rate_a.as<float>(), *wm44 = ctx->ws_rate_b.as<float>(), *wm = ctx->ws_rate_c.as<float>();
  if (int rc = resample_device (ctx, down, pcm_in_d, n_frames, C, x44, n44)) return rc;
  {
    awmk::AddMixArgs a {};
    a.pcm_in = x44;
    a.out = wm44;
    a.n_frames = (long long) n44;
    a.n_channels = C;
    a.frame_mod = frame_mod_dev;
    fill_add_mix_common (a, water_delta);
    a.frames_per_span = frames_per_span (ctx, (long long) (F + 1));
    a.delta_only = 1;
    ProfScope ps (ctx, PROF_ADD_MIX, double (n44) * C * 8.0);
    AWM_HIP_CHECK (awmk::launch_add_mix (ctx->stream, ctx->tabs, a));
  }
  // only frames 0 .. F - 1 of wm44 are complete; nothing later is read (n_in = F * 1024 makes the rest zero, unreachable anyway)
  if (int rc = resample_device (ctx, up, wm44, F * Params::frame_size, C, wm, n_frames)) return rc;
  const int lim_block = int (size_t (rate) * size_t (Params::limiter_block_size_ms) / 1000);
  const size_t n_blocks = n_frames / lim_block + 2;
  unsigned int *block_max = nullptr;
  if (use_limiter)
    {
      if (int rc = ctx->ws_block_max.reserve (n_blocks * sizeof (float))) return rc;
      block_max = ctx->ws_block_max.as<unsigned int>();
      if (int rc = awm_add_init_block_max_d (ctx, ctx->ws_block_max.as<float>(), n_blocks)) return rc;
    }
  AWM_HIP_CHECK (awmk::launch_mix_max (ctx->stream, pcm_in_d, wm, out_d, (long long) n_frames, C, block_max, (long long) n_blocks, lim_block));
  if (ctx->snr_on)
    AWM_HIP_CHECK (awmk::launch_power_sums (ctx->stream, pcm_in_d, out_d, (long long) (n_frames * C), ctx->ws_snr.as<double>()));
  if (use_limiter)
    {
      const size_t tab_entries = awmk::limiter_tab_entries ((long long) n_frames, 0, lim_block);
      if (int rc = ctx->ws_limit_tab.reserve ((tab_entries + 1) * sizeof (float2))) return rc;
      ProfScope ps (ctx, PROF_LIMITER, double (n_frames) * C * 8.0);
      AWM_HIP_CHECK (awmk::launch_limiter (ctx->stream, out_d, (long long) n_frames, C, 0, ctx->ws_block_max.as<float>(), 0, (long long) n_blocks,
                                           lim_block, LIMITER_CEILING, ctx->ws_limit_tab.as<float2>(), tab_entries));
    }
  return 0;
}

static int g_add_payloads_fused = 1, g_add_payloads_fused_in_use = 0;        // (awm_debug_set_add_payloads_fused, below)
static int add_mix_payloads_impl (awm_ctx *ctx, const float *pcm_in_d, float *const *out_d, size_t n_payloads, size_t n_frames, int n_channels,
                                  const int8_t *const *frame_mod_dev, double water_delta, size_t first_frame, const float *halo_before_d,
                                  const float *halo_after_d, float *const *block_max_d, size_t first_block, size_t n_blocks, int delta_only = 0);
struct AddStreamRate;                 // the state of the object at another sample rate (below)
static void add_stream_rate_release (AddStreamRate *r);
static float *add_stream_rate_input (awm_add_stream *s);
static int add_stream_rate_push (awm_add_stream *s, size_t n_frames, int last, const float **out_d, size_t out_frames[3], const char *who);
static awmk::ResampleArgs resample_table_args (const ResampleTable& t, int C);

/* ---- add as a tile loop (reference add_stream_watermark, wmadd.cc:520-589: the stream is processed frame by frame with
 * WatermarkSynth holding one frame back (wmadd.cc:220-222) and the Limiter holding up to two blocks back (limiter.cc:51-64)).
 * Here a TILE of frames is in flight instead of a frame; what is carried from tile to tile is the same state:
 *   - tile t can be mixed once the first frame of tile t + 1 is there (the 3-frame overlap-add needs the next frame's spectrum)
 *     and needs the last frame of tile t - 1,
 *   - tile t can be limited once tile t + 1 is mixed (the ramp of a block needs the maximum of the following block).
 * Three input and three mix slots rotate; block maxima are kept for the whole stream (4 bytes per second). ------------------- */
struct awm_add_stream
{
  awm_ctx  *ctx = nullptr;
  int       C = 0;
  size_t    P = 1;                    // payloads: every tile is mixed and limited once per payload, from one input
  size_t    tile = 0;                 // samples per channel in a full tile (multiple of 1024)
  bool      limiter = true;
  bool      finished = false;
  long long t = 0;                    // tiles pushed so far
  size_t    len[3] = { 0, 0, 0 };     // samples per channel in the input slots
  DevBuffer in[3], block_max;         // block_max: P arrays of n_blocks maxima each, payload p at p * n_blocks
  std::vector<DevBuffer> table;       // [P] a private copy of each payload's frame_mod table
  std::vector<DevBuffer> mix;         // [3][P] mix slot i of payload p at i * P + p
  size_t    n_blocks = 0;             // block maxima allocated (and initialised) per payload
  // a stream that starts `zero_frames` samples into its frame / limiter block grid (add_stream_watermark's zero_frames, reference
  // wmadd.cc:501-526): whole frames of zeros are only counted (WatermarkGen::skip, Limiter::skip), the rest is a prefix of zeros
  size_t    skipped = 0;              // zero_frames rounded down to whole 1024-sample frames
  size_t    prefix = 0;               // zero_frames % 1024: zeros in front of the caller's first sample inside tile 0
  size_t    first_block = 0;          // limiter block of sample `skipped`: block_max[0]
  AddStreamRate *rate = nullptr;      // another sample rate (awm_add_stream_create_rate_at): of the slots above only `mix` is used then
};

static int
add_stream_grow_blocks (awm_add_stream *s, size_t need)
{
  if (need <= s->n_blocks)
    return 0;
  awm_ctx *ctx = s->ctx;
  size_t cap = std::max<size_t> (4096, s->n_blocks * 2);
  while (cap < need)
    cap *= 2;
  DevBuffer bigger;
  if (int rc = bigger.reserve (s->P * cap * sizeof (float))) return rc;
  for (size_t p = 0; p < s->P; p++)
    {
      if (s->n_blocks)
        AWM_HIP_CHECK (hipMemcpyAsync (bigger.as<float>() + p * cap, s->block_max.as<float>() + p * s->n_blocks, s->n_blocks * sizeof (float),
                                       hipMemcpyDeviceToDevice, ctx->stream));
      if (int rc = awm_add_init_block_max_d (ctx, bigger.as<float>() + p * cap + s->n_blocks, cap - s->n_blocks)) return rc;
    }
  AWM_HIP_CHECK (hipStreamSynchronize (ctx->stream));      // the old array may still be read by a queued kernel
  s->block_max.release();
  s->block_max = bigger;
  s->n_blocks = cap;
  return 0;
}

static int
add_stream_create (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads, int n_channels,
                   size_t tile_frames1024, size_t zero_frames, awm_add_stream **out)
{
  auto s = std::make_unique<awm_add_stream>();
  s->ctx = ctx;
  s->C = n_channels;
  s->P = n_payloads;
  s->tile = tile_frames1024 * Params::frame_size;
  s->limiter = !params().test_no_limiter;
  s->prefix = zero_frames % Params::frame_size;
  s->skipped = zero_frames - s->prefix;
  s->first_block = s->skipped / LIMITER_BLOCK;
  s->table.resize (n_payloads);
  s->mix.resize (3 * n_payloads);
  const size_t table_bytes = 2 * mark_block_frame_count() * Params::n_bands;
  auto fail = [&] (int rc) { awm_add_stream_destroy (s.release()); return rc; };
  for (size_t p = 0; p < n_payloads; p++)
    {
      FrameModTable *fm = ctx->get_frame_mod (capi_key (key), payload_hex[p]);
      if (!fm)
        return fail (AWM_ERR_ARG);
      if (int rc = s->table[p].reserve (table_bytes)) return fail (rc);
      // own copy of the table: the context's cache may evict its entry while the stream lives (or while the next table is made)
      if (hipMemcpyAsync (s->table[p].ptr, fm->dev.ptr, table_bytes, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess
          || hipStreamSynchronize (ctx->stream) != hipSuccess)
        return fail (AWM_ERR_HIP);
    }
  // (one frame of room behind a tile: with a prefix the caller's tile lies `prefix` frames into the slot, what hangs over is
  // carried to the next slot -- or, for the last tile, stays: the last tile may be up to prefix frames longer)
  const size_t room = s->prefix ? Params::frame_size : 0;
  for (int i = 0; i < 3; i++)
    {
      if (int rc = s->in[i].reserve ((s->tile + room) * s->C * sizeof (float))) return fail (rc);
      for (size_t p = 0; p < n_payloads; p++)
        if (int rc = s->mix[i * n_payloads + p].reserve ((s->tile + room) * s->C * sizeof (float))) return fail (rc);
    }
  if (s->prefix)
    AWM_HIP_CHECK (hipMemsetAsync (s->in[0].ptr, 0, s->prefix * s->C * sizeof (float), ctx->stream));
  *out = s.release();
  return 0;
}

int
awm_add_stream_create_at (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, int n_channels, size_t tile_frames1024,
                          size_t zero_frames, awm_add_stream **out)
{
  AWM_ENTER (ctx);
  if (!out || n_channels < 1 || tile_frames1024 < 128)
    {
      set_error ("awm_add_stream_create: bad argument (a tile is at least 128 frames: the limiter looks one second ahead)");
      return AWM_ERR_ARG;
    }
  if (!payload_hex)
    payload_hex = "";
  return add_stream_create (ctx, key, &payload_hex, 1, n_channels, tile_frames1024, zero_frames, out);
}

int
awm_add_stream_create (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, int n_channels, size_t tile_frames1024,
                       awm_add_stream **out)
{
  return awm_add_stream_create_at (ctx, key, payload_hex, n_channels, tile_frames1024, 0, out);
}

/* the same object for P payloads (include/awm_hip.h): one input, P tables, P x 3 mix slots, P arrays of block maxima */
int
awm_add_stream_create_payloads_at (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads, int n_channels,
                                   size_t tile_frames1024, size_t zero_frames, awm_add_stream **out)
{
  AWM_ENTER (ctx);
  if (!out || !payload_hex || n_channels < 1 || tile_frames1024 < 128)
    {
      set_error ("awm_add_stream_create_payloads_at: bad argument (a tile is at least 128 frames: the limiter looks one second ahead)");
      return AWM_ERR_ARG;
    }
  if (n_payloads < 1 || n_payloads > AWM_ADD_STREAM_MAX_PAYLOADS)
    {
      set_error (string_printf ("awm_add_stream_create_payloads_at: %zu payloads (1 .. %d are possible)", n_payloads, AWM_ADD_STREAM_MAX_PAYLOADS));
      return AWM_ERR_ARG;
    }
  if (ctx->snr_on)
    {
      set_error ("awm_add_stream_create_payloads_at: not available while the SNR meter is armed (awm_ctx_snr_begin)");
      return AWM_ERR_ARG;
    }
  for (size_t p = 0; p < n_payloads; p++)
    if (!payload_hex[p] || parse_payload (payload_hex[p]).empty())
      {
        set_error (string_printf ("awm_add_stream_create_payloads_at: cannot parse payload '%s' at index %zu", payload_hex[p] ? payload_hex[p] : "(null)", p));
        return AWM_ERR_ARG;
      }
  return add_stream_create (ctx, key, payload_hex, n_payloads, n_channels, tile_frames1024, zero_frames, out);
}

size_t
awm_add_stream_payloads (const awm_add_stream *s)
{
  return s ? s->P : 0;
}

void
awm_add_stream_destroy (awm_add_stream *s)
{
  if (!s)
    return;
  (void) hipSetDevice (s->ctx->device);
  (void) hipStreamSynchronize (s->ctx->stream);
  s->block_max.release();
  for (DevBuffer& b : s->table)
    b.release();
  for (DevBuffer& b : s->mix)
    b.release();
  for (int i = 0; i < 3; i++)
    s->in[i].release();
  add_stream_rate_release (s->rate);
  delete s;
}

float *
awm_add_stream_input (awm_add_stream *s)
{
  if (s && s->rate)
    return add_stream_rate_input (s);
  return s && !s->finished ? s->in[s->t % 3].as<float>() + s->prefix * s->C : nullptr;
}

/* one push for the P payloads of the object: out_d[i * P + p] = finished tile i of payload p */
static int
add_stream_push (awm_add_stream *s, size_t n_frames, int last, const float **out_d, size_t out_frames[3], const char *who)
{
  awm_ctx *ctx = s->ctx;
  if (s->finished || n_frames > s->tile || (!last && n_frames != s->tile))
    {
      set_error (std::string (who) + ": every tile but the last one must be full, nothing may follow the last one");
      return AWM_ERR_ARG;
    }
  if (s->rate)
    return add_stream_rate_push (s, n_frames, last, out_d, out_frames, who);
  const int C = s->C;
  const size_t N = Params::frame_size, P = s->P;
  const long long t = s->t;
  int n_out = 0;
  for (size_t i = 0; i < 3; i++)
    {
      for (size_t p = 0; p < P; p++)
        out_d[i * P + p] = nullptr;
      out_frames[i] = 0;
    }
  auto slot = [&] (long long k) { return int (k % 3); };
  auto mix_tile = [&] (long long k, bool has_next) -> int {
    const size_t n = s->len[slot (k)];
    if (!n)
      return 0;
    const float *before = k > 0 ? s->in[slot (k - 1)].as<float>() + (s->tile - N) * C : nullptr;
    const float *after = has_next ? s->in[slot (k + 1)].as<float>() : nullptr;
    if (P == 1)
      return add_mix_impl (ctx, s->in[slot (k)].as<float>(), s->mix[slot (k)].as<float>(), n, C, s->table[0].as<int8_t>(), params().water_delta,
                           (s->skipped + size_t (k) * s->tile) / N, before, after, s->limiter ? s->block_max.as<float>() : nullptr,
                           s->first_block, s->n_blocks);
    // the forward half of every frame (the halos included) once for the payloads of a pass
    std::vector<float *> outs (P), maxima (P);
    std::vector<const int8_t *> tables (P);
    for (size_t p = 0; p < P; p++)
      {
        outs[p] = s->mix[slot (k) * P + p].as<float>();
        maxima[p] = s->block_max.as<float>() + p * s->n_blocks;
        tables[p] = s->table[p].as<int8_t>();
      }
    return add_mix_payloads_impl (ctx, s->in[slot (k)].as<float>(), outs.data(), P, n, C, tables.data(), params().water_delta,
                                  (s->skipped + size_t (k) * s->tile) / N, before, after, s->limiter ? maxima.data() : nullptr,
                                  s->first_block, s->n_blocks);
  };
  auto limit_tile = [&] (long long k) -> int {
    const size_t n = s->len[slot (k)];
    if (!n)
      return 0;
    if (s->limiter)
      for (size_t p = 0; p < P; p++)
        if (int rc = awm_add_limit_d (ctx, s->mix[slot (k) * P + p].as<float>(), n, C, s->skipped + size_t (k) * s->tile,
                                      s->block_max.as<float>() + p * s->n_blocks, s->first_block, s->n_blocks))
          return rc;
    // (the zeros in front of the caller's first sample are not part of the output: reference wmadd.cc:574-580)
    const size_t cut = k == 0 ? s->prefix : 0;
    if (n > cut)
      {
        for (size_t p = 0; p < P; p++)
          out_d[n_out * P + p] = s->mix[slot (k) * P + p].as<float>() + cut * C;
        out_frames[n_out++] = n - cut;
      }
    return 0;
  };

  // what the slot holds now: the prefix (tile 0: zeros; later: the frames that hung over the previous tile) and the caller's frames
  // (every tile before this one was full, so `prefix` frames always lie in front of the caller's)
  const size_t held = s->prefix + n_frames;
  const size_t len = last ? held : s->tile;                        // (the last tile keeps what hangs over: at most prefix frames)
  s->len[slot (t)] = len;
  if (!last && s->prefix)
    AWM_HIP_CHECK (hipMemcpyAsync (s->in[slot (t + 1)].ptr, s->in[slot (t)].as<float>() + s->tile * C, s->prefix * C * sizeof (float),
                                   hipMemcpyDeviceToDevice, ctx->stream));
  if (len && len < N)                 // a next tile shorter than a frame: the halo the previous tile reads is zero extended
    AWM_HIP_CHECK (hipMemsetAsync (s->in[slot (t)].as<float>() + len * C, 0, (N - len) * C * sizeof (float), ctx->stream));
  if (s->limiter)
    if (int rc = add_stream_grow_blocks (s, (s->skipped + size_t (t) * s->tile + len) / LIMITER_BLOCK + 2 - s->first_block)) return rc;
  if (t >= 1)
    if (int rc = mix_tile (t - 1, len > 0)) return rc;
  if (t >= 2)
    if (int rc = limit_tile (t - 2)) return rc;
  if (last)
    {
      if (int rc = mix_tile (t, false)) return rc;
      if (t >= 1)
        if (int rc = limit_tile (t - 1)) return rc;
      if (int rc = limit_tile (t)) return rc;
      s->finished = true;
    }
  s->t++;
  return n_out;
}

int
awm_add_stream_push (awm_add_stream *s, size_t n_frames, int last, const float *out_d[3], size_t out_frames[3])
{
  if (!s || !out_d || !out_frames)
    {
      set_error ("awm_add_stream_push: bad argument");
      return AWM_ERR_ARG;
    }
  awm_ctx *ctx = s->ctx;
  AWM_ENTER (ctx);
  if (s->P != 1)
    {
      set_error (string_printf ("awm_add_stream_push: the object has %zu payloads (awm_add_stream_push_payloads)", s->P));
      return AWM_ERR_ARG;
    }
  return add_stream_push (s, n_frames, last, out_d, out_frames, "awm_add_stream_push");
}

int
awm_add_stream_push_payloads (awm_add_stream *s, size_t n_frames, int last, const float **out_d, size_t out_frames[3])
{
  if (!s || !out_d || !out_frames)
    {
      set_error ("awm_add_stream_push_payloads: bad argument");
      return AWM_ERR_ARG;
    }
  awm_ctx *ctx = s->ctx;
  AWM_ENTER (ctx);
  if (ctx->snr_on && s->P > 1)
    {
      set_error ("awm_add_stream_push_payloads: not available while the SNR meter is armed (awm_ctx_snr_begin)");
      return AWM_ERR_ARG;
    }
  return add_stream_push (s, n_frames, last, out_d, out_frames, "awm_add_stream_push_payloads");
}

/* ---- the tile loop at another sample rate (include/awm_hip.h).  add_full_rate's stages at GLOBAL sample and frame
 * indices, each continuing where the previous push stopped:
 *   down (K10s)  the 44.1 kHz samples whose windows lie in what has been pushed, up to a multiple of np;
 *   K2 / K2m     the watermark signal alone for the whole frames that became available but the last, which is the halo behind them (the
 *                frame in front of them is the halo before): a frame's signal is complete once the next frame was transformed;
 *   up (K10s)    per payload, the outputs whose windows lie in complete frames, up to a multiple of np, into one scratch buffer;
 *   K11          scratch + input -> the mix slots of the tiles the run crosses, with the block maxima (in front of the stream the stretch
 *                mix_first .. zero_frames - 1 of watermark alone, which only counts for the maxima);
 *   K3           tile t - 2, once the limiter block behind its last sample is mixed.
 * Every buffer is linear: it holds the samples base .. end - 1 of its stream, and after a push what the next push still reads is copied to
 * the front of its twin (the input that the next windows and the next mix reach back to, two 44.1 kHz frames and the remainder, the
 * watermark samples the next up window starts in).  awm_add_stream_rate_plan says how far the mix lags behind the input. ---- */
struct AddStreamRate
{
  int       rate = 0;
  awm_stream_rate_plan plan {};
  const ResampleTable *down = nullptr, *up = nullptr;
  uint64_t  Z = 0;                                // zero_frames: sample of the stream where the caller's first sample lies
  uint64_t  mix_first = 0, frame_first = 0, slice_first = 0;          // awm_add_segment_plan's, which depend on Z alone
  DevBuffer in[2];                                // the stream at the rate: in[in_cur] holds samples in_base .. in_end - 1, the caller writes behind them
  int       in_cur = 0;
  uint64_t  in_base = 0, in_end = 0;
  size_t    in_cap = 0;                           // samples per channel each of them takes
  DevBuffer x44[2];                               // the stream at 44.1 kHz: x44[x_cur] holds samples x_base .. d_done - 1
  int       x_cur = 0;
  uint64_t  x_base = 0, d_done = 0;
  size_t    cap44 = 0;
  std::vector<DevBuffer> wm44;                    // [2][P] the watermark at 44.1 kHz: wm44[w_cur * P + p] holds samples w_base .. w_end - 1
  int       w_cur = 0;
  uint64_t  w_base = 0, w_end = 0;                // w_end = k_done * 1024: the end of the complete frames
  uint64_t  k_done = 0;                           // the next frame K2 produces
  DevBuffer wm;                                   // the watermark at the rate for the outputs of one push (one payload after the other)
  size_t    wm_cap = 0;
  uint64_t  u_done = 0;                           // the next output to be mixed
  long long limited = 0;                          // tiles handed out so far
  DevBuffer limit_tab;
  size_t    tab_entries = 0;
};

static void
add_stream_rate_release (AddStreamRate *r)
{
  if (!r)
    return;
  for (int i = 0; i < 2; i++)
    {
      r->in[i].release();
      r->x44[i].release();
    }
  for (DevBuffer& b : r->wm44)
    b.release();
  r->wm.release();
  r->limit_tab.release();
  delete r;
}

static float *
add_stream_rate_input (awm_add_stream *s)
{
  AddStreamRate *r = s->rate;
  return s->finished ? nullptr : r->in[r->in_cur].as<float>() + (r->in_end - r->in_base) * s->C;
}

// what the next push still reads of a linear buffer: samples new_base .. end - 1 to the front of its twin
static int
add_stream_rate_carry (hipStream_t st, const DevBuffer& from, DevBuffer& to, uint64_t base, uint64_t new_base, uint64_t end, int C)
{
  if (end > new_base)
    AWM_HIP_CHECK (hipMemcpyAsync (to.ptr, from.as<float>() + (new_base - base) * C, (end - new_base) * C * sizeof (float),
                                   hipMemcpyDeviceToDevice, st));
  return 0;
}

static int
add_stream_create_rate (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads, int n_channels, int sample_rate,
                        size_t tile_frames1024, size_t zero_frames, awm_add_stream **out, const char *who)
{
  awm_stream_rate_plan plan;
  if (int rc = awm_add_stream_rate_plan (sample_rate, &plan))
    return rc;
  constexpr uint64_t LIMIT = uint64_t (1) << 40;
  if (tile_frames1024 >= LIMIT / Params::frame_size || tile_frames1024 * Params::frame_size < plan.min_tile)
    {
      set_error (string_printf ("%s: a tile of %zu samples at %d Hz (min_tile, awm_add_stream_rate_plan: %llu samples; at most 2^40)", who,
                                tile_frames1024 * Params::frame_size, sample_rate, (unsigned long long) plan.min_tile));
      return AWM_ERR_ARG;
    }
  if (ctx->snr_on)
    {
      set_error (std::string (who) + ": not available at this sample rate while the SNR meter is armed (awm_ctx_snr_begin)");
      return AWM_ERR_ARG;
    }
  awm_segment_plan sp;
  if (int rc = awm_add_segment_plan (sample_rate, zero_frames, 1, &sp))          // (refuses zero_frames + 1 >= 2^40)
    return rc;
  auto s = std::make_unique<awm_add_stream>();
  s->ctx = ctx;
  s->C = n_channels;
  s->P = n_payloads;
  s->tile = tile_frames1024 * Params::frame_size;
  s->limiter = !params().test_no_limiter;
  s->first_block = size_t (sp.first_block);
  s->table.resize (n_payloads);
  s->mix.resize (3 * n_payloads);
  AddStreamRate *r = s->rate = new AddStreamRate;
  auto fail = [&] (int rc) { awm_add_stream_destroy (s.release()); return rc; };
  const size_t table_bytes = 2 * mark_block_frame_count() * Params::n_bands;
  for (size_t p = 0; p < n_payloads; p++)
    {
      FrameModTable *fm = ctx->get_frame_mod (capi_key (key), payload_hex[p]);
      if (!fm)
        return fail (AWM_ERR_ARG);
      if (int rc = s->table[p].reserve (table_bytes)) return fail (rc);
      if (hipMemcpyAsync (s->table[p].ptr, fm->dev.ptr, table_bytes, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess
          || hipStreamSynchronize (ctx->stream) != hipSuccess)
        return fail (AWM_ERR_HIP);
    }
  r->rate = sample_rate;
  r->plan = plan;
  r->down = ctx->get_resample_table (sample_rate, Params::mark_sample_rate);
  r->up = ctx->get_resample_table (Params::mark_sample_rate, sample_rate);
  if (!r->down || !r->up)
    return fail (AWM_ERR_HIP);
  r->Z = zero_frames;
  r->mix_first = sp.mix_first;
  r->frame_first = sp.frame_first;
  r->slice_first = sp.slice_first;
  r->in_base = r->in_end = zero_frames;
  r->x_base = r->d_done = sp.down_first;
  r->k_done = sp.slice_first;
  r->w_base = r->w_end = sp.slice_first * Params::frame_size;
  r->u_done = sp.mix_first;
  // room: a tile and what is carried.  The mix lags at most mix_ahead + down_step + up_np + 1 behind the input (the launches end on
  // multiples of np), the watermark in front of the stream is shorter than mix_ahead, the flush adds two frames and the windows
  const size_t slack = size_t (plan.mix_ahead) + 2 * size_t (plan.down_hl) + 4 * size_t (plan.down_step) + 2 * size_t (plan.up_np) + Params::frame_size;
  r->in_cap = s->tile + slack;
  r->cap44 = size_t (s->tile * uint64_t (plan.down_np) / uint64_t (plan.down_step)) + 8 * Params::frame_size + 2 * size_t (plan.down_np) + 64;
  r->wm_cap = s->tile + size_t (plan.mix_ahead) + slack;
  r->tab_entries = s->tile / size_t (plan.limiter_block) + 3;
  const size_t C = size_t (n_channels);
  r->wm44.resize (2 * n_payloads);
  for (int i = 0; i < 2; i++)
    {
      if (int rc = r->in[i].reserve (r->in_cap * C * sizeof (float))) return fail (rc);
      if (int rc = r->x44[i].reserve (r->cap44 * C * sizeof (float))) return fail (rc);
      for (size_t p = 0; p < n_payloads; p++)
        if (int rc = r->wm44[i * n_payloads + p].reserve (r->cap44 * C * sizeof (float))) return fail (rc);
    }
  if (int rc = r->wm.reserve (r->wm_cap * C * sizeof (float))) return fail (rc);
  if (int rc = r->limit_tab.reserve ((r->tab_entries + 1) * sizeof (float2))) return fail (rc);
  for (size_t i = 0; i < 3 * n_payloads; i++)
    if (int rc = s->mix[i].reserve (s->tile * C * sizeof (float))) return fail (rc);
  if (s->limiter)                                            // the first 4096 block maxima (68 minutes) now: a push allocates only beyond them
    if (int rc = add_stream_grow_blocks (s.get(), 1)) return fail (rc);
  *out = s.release();
  return 0;
}

static int
add_stream_rate_push (awm_add_stream *s, size_t n_frames, int last, const float **out_d, size_t out_frames[3], const char *who)
{
  awm_ctx *ctx = s->ctx;
  AddStreamRate *r = s->rate;
  hipStream_t st = ctx->stream;
  const size_t C = size_t (s->C), P = s->P, FRAME = Params::frame_size;
  const awm_stream_rate_plan& pl = r->plan;
  const uint64_t Z = r->Z, tile = s->tile, B = pl.limiter_block;
  const uint64_t hd = uint64_t (pl.down_hl), nd = uint64_t (pl.down_np), sd = uint64_t (pl.down_step);
  const uint64_t hu = uint64_t (pl.up_hl), nu = uint64_t (pl.up_np), su = uint64_t (pl.up_step);
  for (size_t i = 0; i < 3; i++)
    {
      for (size_t p = 0; p < P; p++)
        out_d[i * P + p] = nullptr;
      out_frames[i] = 0;
    }
  if (ctx->snr_on)
    {
      set_error (std::string (who) + ": not available at this sample rate while the SNR meter is armed (awm_ctx_snr_begin)");
      return AWM_ERR_ARG;
    }
  if (r->in_end + n_frames >= (uint64_t (1) << 40))
    {
      set_error (std::string (who) + ": zero_frames + the samples pushed must stay below 2^40");
      return AWM_ERR_ARG;
    }
  auto internal = [&] (const char *what) {
    set_error (std::string (who) + ": " + what + " (the tile is too short for this sample rate: awm_add_stream_rate_plan)");
    return AWM_ERR_GENERIC;
  };
  // the windows: output m of a resampler reads inputs floor (m step / np) - hl + 1 ... floor (m step / np) + hl
  auto window_first = [] (uint64_t m, uint64_t hl, uint64_t step, uint64_t np) { const uint64_t b = m * step / np; return b + 1 > hl ? b + 1 - hl : 0; };
  auto outputs_within = [] (uint64_t end, uint64_t hl, uint64_t step, uint64_t np) {        // how many outputs read nothing from `end` on
    return end > hl ? ((end - hl) * np + step - 1) / step : uint64_t (0);
  };
  r->in_end += n_frames;
  const uint64_t in_end = r->in_end;
  if (last && in_end == Z)                                   // nothing was ever pushed
    {
      s->finished = true;
      s->t++;
      return 0;
    }
  if (s->limiter)
    if (int rc = add_stream_grow_blocks (s, size_t (in_end / B + 2 - s->first_block))) return rc;
  const float *in = r->in[r->in_cur].as<float>();
  float *x44 = r->x44[r->x_cur].as<float>();

  // 1. down.  At the end of the stream: the frames the last output's window reaches, and the frame behind them
  uint64_t d_new;
  if (last)
    d_new = ((((in_end - 1) * su / nu + hu) / FRAME) + 2) * FRAME;
  else
    d_new = outputs_within (in_end, hd, sd, nd) / nd * nd;
  d_new = std::max (d_new, r->d_done);
  if (d_new > r->d_done)
    {
      if (d_new - r->x_base > r->cap44)
        return internal ("the 44.1 kHz slot is full");
      const awmk::ResampleSlice sl { in, (long long) (in_end - r->in_base), (long long) r->in_base, (long long) r->d_done,
                                     (long long) (d_new - r->d_done), x44 + (r->d_done - r->x_base) * C };
      ProfScope ps (ctx, PROF_RESAMPLE, double (sl.n_in + sl.n_out) * C * 4.0);
      AWM_HIP_CHECK (awmk::launch_resample_span (st, resample_table_args (*r->down, int (C)), sl));
    }
  r->d_done = d_new;

  // 2. the watermark signal of the frames k_done .. fb - 2; frame fb - 1 is the halo behind them
  const uint64_t fb = d_new / FRAME;
  if (fb > r->k_done + 1)
    {
      const uint64_t k0 = r->k_done, k1 = fb - 1;
      if (k1 * FRAME - r->w_base > r->cap44)
        return internal ("the watermark slot is full");
      const float *before = k0 > r->slice_first ? x44 + ((k0 - 1) * FRAME - r->x_base) * C : nullptr;
      const float *after = x44 + (k1 * FRAME - r->x_base) * C;
      const float *src = x44 + (k0 * FRAME - r->x_base) * C;
      std::vector<float *> outs (P);
      std::vector<const int8_t *> tables (P);
      for (size_t p = 0; p < P; p++)
        {
          outs[p] = r->wm44[r->w_cur * P + p].as<float>() + (k0 * FRAME - r->w_base) * C;
          tables[p] = s->table[p].as<int8_t>();
        }
      if (P == 1)
        {
          if (int rc = add_mix_impl (ctx, src, outs[0], size_t ((k1 - k0) * FRAME), int (C), tables[0], params().water_delta, size_t (k0), before,
                                     after, nullptr, 0, 0, nullptr, 1))
            return rc;
        }
      else if (int rc = add_mix_payloads_impl (ctx, src, outs.data(), P, size_t ((k1 - k0) * FRAME), int (C), tables.data(), params().water_delta,
                                               size_t (k0), before, after, nullptr, 0, 0, 1))
        return rc;
      r->k_done = k1;
      r->w_end = k1 * FRAME;
    }

  // 3. up and mix, per payload: the outputs whose windows lie in complete frames
  uint64_t u_new;
  if (last)
    {
      u_new = in_end;
      if (outputs_within (r->w_end, hu, su, nu) < u_new)
        return internal ("the last frames are missing");
    }
  else
    u_new = std::min (outputs_within (r->w_end, hu, su, nu), in_end) / nu * nu;
  u_new = std::max (u_new, r->u_done);
  if (u_new > r->u_done)
    {
      const uint64_t u0 = r->u_done;
      if (u_new - u0 > r->wm_cap)
        return internal ("the watermark signal's slot is full");
      if (std::max (u0, Z) < r->in_base)
        return internal ("the input of the mix is gone");
      const uint64_t res0 = std::max (r->w_base, r->frame_first * FRAME);        // only complete frames are handed over
      if (r->w_end < res0)
        return internal ("no complete frame");
      float *wm = r->wm.as<float>();
      for (size_t p = 0; p < P; p++)
        {
          {
            const awmk::ResampleSlice sl { r->wm44[r->w_cur * P + p].as<float>() + (res0 - r->w_base) * C, (long long) (r->w_end - res0), (long long) res0,
                                           (long long) u0, (long long) (u_new - u0), wm };
            ProfScope ps (ctx, PROF_RESAMPLE, double (sl.n_in + sl.n_out) * C * 4.0);
            AWM_HIP_CHECK (awmk::launch_resample_span (st, resample_table_args (*r->up, int (C)), sl));
          }
          unsigned int *block_max = s->limiter ? s->block_max.as<unsigned int>() + p * s->n_blocks : nullptr;
          for (uint64_t a = u0; a < u_new; )                 // one piece per tile the run crosses
            {
              const uint64_t lo = std::max (a, Z), k = (lo - Z) / tile;
              const uint64_t b = std::min (u_new, Z + (k + 1) * tile);
              const uint64_t n = b > lo ? b - lo : 0, pre = a < Z ? std::min (b, Z) - a : 0;
              if (n && (long long) k >= r->limited + 3)
                return internal ("a mix slot is still in use");
              const awmk::MixSegment ms { in + (lo - r->in_base) * C, wm + (a - u0) * C, s->mix[(k % 3) * P + p].as<float>() + (lo - (Z + k * tile)) * C,
                                          (long long) n, (long long) pre, (long long) (a + pre), block_max, (long long) s->first_block,
                                          (long long) s->n_blocks };
              AWM_HIP_CHECK (awmk::launch_mix_max_segment (st, ms, int (C), int (B)));
              a = b;
            }
        }
    }
  r->u_done = u_new;

  // 4. the limiter: a tile's last sample needs the maximum of the limiter block behind its own
  int n_out = 0;
  const long long t = s->t;
  while (r->limited <= t)
    {
      const uint64_t k = uint64_t (r->limited), t0 = Z + k * tile, t1 = std::min (t0 + tile, in_end);
      const uint64_t n = t1 > t0 ? t1 - t0 : 0;
      if (!last && (n < tile || u_new < ((t1 - 1) / B + 2) * B))
        break;
      if (n)
        {
          if (n_out == 3)
            return internal ("more than three tiles became final");
          for (size_t p = 0; p < P; p++)
            {
              float *data = s->mix[(k % 3) * P + p].as<float>();
              if (s->limiter)
                {
                  ProfScope ps (ctx, PROF_LIMITER, double (n) * C * 8.0);
                  AWM_HIP_CHECK (awmk::launch_limiter (st, data, (long long) n, int (C), (long long) t0, s->block_max.as<float>() + p * s->n_blocks,
                                                       (long long) s->first_block, (long long) s->n_blocks, int (B), LIMITER_CEILING,
                                                       r->limit_tab.as<float2>(), r->tab_entries));
                }
              out_d[n_out * P + p] = data;
            }
          out_frames[n_out++] = size_t (n);
        }
      r->limited++;
    }
  if (!last && t >= 2 && r->limited < t - 1)
    return internal ("a tile is not final two pushes after its own");

  // 5. what the next push reads, to the front of the twins
  if (last)
    s->finished = true;
  else
    {
      {
        const uint64_t from = std::max (std::min (window_first (d_new, hd, sd, nd), u_new), r->in_base);      // the next windows, the next mix
        const uint64_t keep = from < in_end ? (in_end - from + 3) / 4 * 4 : 0;        // the caller's pointer stays 16-byte aligned
        if (keep > in_end - r->in_base || keep + tile > r->in_cap)
          return internal ("the input slot is full");
        if (int rc = add_stream_rate_carry (st, r->in[r->in_cur], r->in[r->in_cur ^ 1], r->in_base, in_end - keep, in_end, int (C))) return rc;
        r->in_base = in_end - keep;
        r->in_cur ^= 1;
      }
      {
        const uint64_t from = r->k_done > r->slice_first ? (r->k_done - 1) * FRAME : r->x_base;
        if (int rc = add_stream_rate_carry (st, r->x44[r->x_cur], r->x44[r->x_cur ^ 1], r->x_base, from, d_new, int (C))) return rc;
        r->x_base = from;
        r->x_cur ^= 1;
      }
      {
        const uint64_t from = std::min (std::max (window_first (u_new, hu, su, nu), r->w_base), r->w_end);
        for (size_t p = 0; p < P; p++)
          if (int rc = add_stream_rate_carry (st, r->wm44[r->w_cur * P + p], r->wm44[(r->w_cur ^ 1) * P + p], r->w_base, from, r->w_end, int (C)))
            return rc;
        r->w_base = from;
        r->w_cur ^= 1;
      }
    }
  s->t++;
  return n_out;
}

static int
add_stream_rate_args_ok (const char *who, const void *out, int n_channels, int sample_rate, size_t tile_frames1024)
{
  if (!out || n_channels < 1 || tile_frames1024 < 128)
    {
      set_error (std::string (who) + ": bad argument (a tile is at least 128 frames: the limiter looks one second ahead)");
      return AWM_ERR_ARG;
    }
  if (sample_rate <= 0)
    {
      set_error (string_printf ("%s: sample_rate %d", who, sample_rate));
      return AWM_ERR_ARG;
    }
  return 0;
}

int
awm_add_stream_create_rate_at (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, int n_channels, int sample_rate,
                               size_t tile_frames1024, size_t zero_frames, awm_add_stream **out)
{
  if (sample_rate == Params::mark_sample_rate)
    return awm_add_stream_create_at (ctx, key, payload_hex, n_channels, tile_frames1024, zero_frames, out);
  AWM_ENTER (ctx);
  if (int rc = add_stream_rate_args_ok ("awm_add_stream_create_rate_at", out, n_channels, sample_rate, tile_frames1024))
    return rc;
  if (!payload_hex)
    payload_hex = "";
  return add_stream_create_rate (ctx, key, &payload_hex, 1, n_channels, sample_rate, tile_frames1024, zero_frames, out, "awm_add_stream_create_rate_at");
}

int
awm_add_stream_create_payloads_rate_at (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads, int n_channels,
                                        int sample_rate, size_t tile_frames1024, size_t zero_frames, awm_add_stream **out)
{
  if (sample_rate == Params::mark_sample_rate)
    return awm_add_stream_create_payloads_at (ctx, key, payload_hex, n_payloads, n_channels, tile_frames1024, zero_frames, out);
  AWM_ENTER (ctx);
  const char *who = "awm_add_stream_create_payloads_rate_at";
  if (int rc = add_stream_rate_args_ok (who, payload_hex ? (const void *) out : nullptr, n_channels, sample_rate, tile_frames1024))
    return rc;
  if (n_payloads < 1 || n_payloads > AWM_ADD_STREAM_MAX_PAYLOADS)
    {
      set_error (string_printf ("%s: %zu payloads (1 .. %d are possible)", who, n_payloads, AWM_ADD_STREAM_MAX_PAYLOADS));
      return AWM_ERR_ARG;
    }
  for (size_t p = 0; p < n_payloads; p++)
    if (!payload_hex[p] || parse_payload (payload_hex[p]).empty())
      {
        set_error (string_printf ("%s: cannot parse payload '%s' at index %zu", who, payload_hex[p] ? payload_hex[p] : "(null)", p));
        return AWM_ERR_ARG;
      }
  return add_stream_create_rate (ctx, key, payload_hex, n_payloads, n_channels, sample_rate, tile_frames1024, zero_frames, out, who);
}

int
awm_add_stream_sample_rate (const awm_add_stream *s)
{
  return !s ? 0 : s->rate ? s->rate->rate : Params::mark_sample_rate;
}

int
awm_debug_resample_span_d (awm_ctx *ctx, const float *in_d, size_t n_in, uint64_t in0, uint64_t out0, size_t n_out, int n_channels,
                           int rate_in, int rate_out, float *out_d, int *phase_form_used)
{
  AWM_ENTER (ctx);
  constexpr uint64_t LIMIT = uint64_t (1) << 41;             // K10w: m step in 64 bits
  if ((n_in && !in_d) || (n_out && !out_d) || n_channels < 1 || in0 >= LIMIT || n_in >= LIMIT || out0 >= LIMIT || n_out >= LIMIT)
    {
      set_error ("awm_debug_resample_span_d: bad argument");
      return AWM_ERR_ARG;
    }
  const ResampleTable *t = rate_in > 0 && rate_out > 0 ? ctx->get_resample_table (rate_in, rate_out) : nullptr;
  if (!t)
    {
      set_error (string_printf ("awm_debug_resample_span_d: no fixed-ratio resampler from %d Hz to %d Hz", rate_in, rate_out));
      return AWM_ERR_ARG;
    }
  const awmk::ResampleArgs ra = resample_table_args (*t, n_channels);
  const awmk::ResampleSlice sl { in_d, (long long) n_in, (long long) in0, (long long) out0, (long long) n_out, out_d };
  if (phase_form_used)
    *phase_form_used = n_out && awmk::resample_span_takes_phase (ra, sl) ? 1 : 0;
  ProfScope ps (ctx, PROF_RESAMPLE, double (n_in + n_out) * n_channels * 4.0);
  AWM_HIP_CHECK (awmk::launch_resample_span (ctx->stream, ra, sl));
  return 0;
}

int
awm_add_d (awm_ctx *ctx, const float *pcm_in_d, float *out_d, size_t n_frames, int n_channels,
           const int8_t *frame_mod, double water_delta, int use_limiter)
{
  AWM_ENTER (ctx);
  if (!pcm_in_d || !out_d || !frame_mod || n_channels < 1)
    {
      set_error ("awm_add_d: bad argument");
      return AWM_ERR_ARG;
    }
  if (add_buffers_overlap (pcm_in_d, out_d, n_frames * size_t (n_channels)))
    {
      set_error ("awm_add_d: the output overlaps the input");
      return AWM_ERR_ARG;
    }
  const size_t table_bytes = 2 * mark_block_frame_count() * Params::n_bands;
  if (int rc = ctx->ws_misc.reserve (table_bytes)) return rc;
  AWM_HIP_CHECK (hipMemcpyAsync (ctx->ws_misc.ptr, frame_mod, table_bytes, hipMemcpyHostToDevice, ctx->stream));
  return add_full (ctx, pcm_in_d, out_d, n_frames, n_channels, ctx->ws_misc.as<int8_t>(), water_delta, use_limiter);
}

static bool
pcm_format_ok (int bit_depth, int encoding)
{
  if (encoding == 2)
    return bit_depth == 32 || bit_depth == 64;
  return (encoding == 0 || encoding == 1) && (bit_depth == 8 || bit_depth == 16 || bit_depth == 24 || bit_depth == 32);
}

int
awm_pcm_decode_d (awm_ctx *ctx, const void *bytes_d, size_t n_values, int bit_depth, int encoding, int big_endian, float *out_d)
{
  AWM_ENTER (ctx);
  if (!pcm_format_ok (bit_depth, encoding))
    {
      set_error ("awm_pcm_decode_d: unsupported sample format");
      return AWM_ERR_ARG;
    }
  const awmk::PcmFormatDev f { bit_depth / 8, encoding, big_endian != 0, 0 };
  ProfScope ps (ctx, PROF_PCM_DECODE, double (n_values) * (bit_depth / 8 + 4));
  AWM_HIP_CHECK (awmk::launch_pcm_decode (ctx->stream, static_cast<const unsigned char *> (bytes_d), out_d, (long long) n_values, f));
  return 0;
}

int
awm_pcm_encode_d (awm_ctx *ctx, const float *in_d, size_t n_values, int bit_depth, int encoding, int big_endian, int direct16, void *bytes_d)
{
  AWM_ENTER (ctx);
  if (!pcm_format_ok (bit_depth, encoding))
    {
      set_error ("awm_pcm_encode_d: unsupported sample format");
      return AWM_ERR_ARG;
    }
  const bool d16 = direct16 && bit_depth == 16 && encoding == 0 && !big_endian;
  const awmk::PcmFormatDev f { bit_depth / 8, encoding, big_endian != 0, d16 };
  ProfScope ps (ctx, PROF_PCM_ENCODE, double (n_values) * (bit_depth / 8 + 4));
  AWM_HIP_CHECK (awmk::launch_pcm_encode (ctx->stream, in_d, static_cast<unsigned char *> (bytes_d), (long long) n_values, f));
  return 0;
}

static int g_k4s_ablate = 0;
extern "C" void awm_debug_set_k4s_ablate (int f) { g_k4s_ablate = f; }
int
awm_debug_sync_db_sliding_d (awm_ctx *ctx, const float *pcm_d, size_t n_frames, int n_channels, const long long *base_d, size_t n_streams,
                             int count, int ld, float *out_d)
{
  AWM_ENTER (ctx);
  if (!pcm_d || !base_d || !out_d || count < 1 || count > 65 || (ld < count && ld != 64) || (n_channels != 1 && n_channels != 2))
    {
      set_error ("awm_debug_sync_db_sliding_d: bad argument");
      return AWM_ERR_ARG;
    }
  awmk::SyncDbArgs da {};
  da.pcm = pcm_d;
  da.n_frames = (long long) n_frames;
  da.n_channels = n_channels;
  da.stream_base = base_d;
  da.count0 = count;
  da.n_streams = (long long) n_streams;
  da.hop = Params::sync_search_fine;
  da.out = out_d;
  da.out_stream_stride = (long long) Params::n_bands * ld;
  da.ld = ld;
  da.first = 0;
  da.last = (long long) (n_frames * n_channels);
  da.tile_frames = ld;
  da.xcd_interleave = g_k4s_ablate;
  if (ld == 64)
    {
      // (measurement, tools/gpu_k4s_alone.py: the refinement's gathered layout with a synthetic table -- bands 0..59 are the rows --, rows
      // of 64 offsets at out_d[i][60][64] and the 65th values behind them at out_d + n_streams * 60 * 64)
      std::vector<unsigned char> pos (Params::n_bands, 255);
      for (int b = 0; b < 60; b++)
        pos[b] = (unsigned char) b;
      if (int rc = ctx->ws_misc.reserve (Params::n_bands + sizeof (int))) return rc;
      const int zero = 0;
      AWM_HIP_CHECK (hipMemcpyAsync (ctx->ws_misc.ptr, &zero, sizeof (int), hipMemcpyHostToDevice, ctx->stream));
      AWM_HIP_CHECK (hipMemcpyAsync (ctx->ws_misc.as<char>() + sizeof (int), pos.data(), pos.size(), hipMemcpyHostToDevice, ctx->stream));
      da.row_perm = ctx->ws_misc.as<int>();
      da.band_pos = ctx->ws_misc.as<unsigned char>() + sizeof (int);
      da.rows_per_plane = 1;
      da.out_stream_stride = 60 * 64;
      if (awmk::sliding_rows_have_tail (n_channels))
        {
          da.tail = out_d + n_streams * 60 * 64;
          da.tail_stream_stride = 60;
        }
      else if (count > 64)
        {
          set_error ("awm_debug_sync_db_sliding_d: rows of 64 offsets take 65 only with forms 4 / 5");
          return AWM_ERR_ARG;
        }
    }
  AWM_HIP_CHECK (awmk::launch_sync_db_sliding (ctx->stream, ctx->tabs, da));
  return 0;
}

/* the body of awm_debug_sync_db_sliding_rows_d and of its 16-bit twin (s16: pcm_d holds the address of int16 values) */
static int
sliding_rows_body (awm_ctx *ctx, const char *who, const void *pcm_d, bool s16, size_t n_frames, int n_channels, const long long *base_d, const int *count_d,
                   size_t n_streams, int count0, int rows_per_plane, const int *row_perm_d, const unsigned char *band_pos_d,
                   long long first, long long last, const long long *stream_range_d, const int *range_index_d, int range_div,
                   int tables_per_slice, int ld, float *out_d, float *tail_d, long long tail_stream_stride, char *have_d,
                   long long have_stream_stride)
{
  const char *bad = nullptr;
  if (!pcm_d || !base_d || !count_d || !row_perm_d || !band_pos_d || !out_d || !have_d)
    bad = "null pointer";
  else if (n_channels != 1 && n_channels != 2)
    bad = "1 or 2 channels";
  else if (count0 < 0 || count0 > 65 || have_stream_stride < count0)
    bad = "count0 within 0 .. 65 and within a stream's have flags";
  else if (rows_per_plane < 1 || range_div < 1 || (tables_per_slice != 0 && tables_per_slice != 1))
    bad = "rows_per_plane, range_div or tables_per_slice";
  else if (tail_d && (!awmk::sliding_rows_have_tail (n_channels) || tail_stream_stride < 60))
    bad = "only forms 4 / 5 write a tail (stereo), 60 values per stream";
  else if (ld < std::min (count0, tail_d ? 64 : 65))
    bad = "ld below the offsets of a row (64 only with a tail)";
  if (!bad && n_streams)
    {
      // what the kernels take on trust from the refinement (syncfinder.cc:520-551): counts within count0, every window inside the stream
      std::vector<long long> base (n_streams);
      std::vector<int> count (n_streams);
      AWM_HIP_CHECK (hipMemcpyAsync (base.data(), base_d, n_streams * sizeof (long long), hipMemcpyDeviceToHost, ctx->stream));
      AWM_HIP_CHECK (hipMemcpyAsync (count.data(), count_d, n_streams * sizeof (int), hipMemcpyDeviceToHost, ctx->stream));
      AWM_HIP_CHECK (hipStreamSynchronize (ctx->stream));
      for (size_t s = 0; s < n_streams && !bad; s++)
        {
          if (count[s] < 0 || count[s] > count0)
            bad = "a stream's count outside 0 .. count0";
          else if (count[s] && (base[s] < 0 || base[s] + 8LL * (count[s] - 1) + (long long) Params::frame_size > (long long) n_frames))
            bad = "a stream's windows outside the samples";
        }
    }
  if (bad)
    {
      set_error (std::string (who) + ": " + bad);
      return AWM_ERR_ARG;
    }
  // (the fields and their order: SyncFinder's refinement, syncfinder.cc "K4s: sliding DFT over the fine offsets")
  awmk::SyncDbArgs da {};
  da.pcm = static_cast<const float *> (pcm_d);
  da.n_frames = (long long) n_frames;
  da.n_channels = n_channels;
  da.per_channel = 0;
  da.stream_base = base_d;
  da.stream_count = count_d;
  da.count0 = count0;
  da.n_streams = (long long) n_streams;
  da.hop = Params::sync_search_fine;
  da.out = out_d;
  da.out_stream_stride = 60LL * ld;
  da.row_perm = row_perm_d;
  da.band_pos = band_pos_d;
  da.rows_per_plane = rows_per_plane;
  da.ld = ld;
  da.tail = tail_d;
  da.tail_stream_stride = tail_stream_stride;
  da.have = have_d;
  da.have_stream_stride = have_stream_stride;
  da.first = first;
  da.last = last;
  if (stream_range_d || tables_per_slice)
    {
      da.stream_range = stream_range_d;
      da.range_index = range_index_d;
      da.range_div = range_div;
      da.tables_per_slice = tables_per_slice;
    }
  da.tile_frames = ld;
  if (s16)
    AWM_HIP_CHECK (awmk::launch_sync_db_sliding_s16 (ctx->stream, ctx->tabs, da));
  else
    AWM_HIP_CHECK (awmk::launch_sync_db_sliding (ctx->stream, ctx->tabs, da));
  return 0;
}

int
awm_debug_sync_db_sliding_rows_d (awm_ctx *ctx, const float *pcm_d, size_t n_frames, int n_channels, const long long *base_d, const int *count_d,
                                  size_t n_streams, int count0, int rows_per_plane, const int *row_perm_d, const unsigned char *band_pos_d,
                                  long long first, long long last, const long long *stream_range_d, const int *range_index_d, int range_div,
                                  int tables_per_slice, int ld, float *out_d, float *tail_d, long long tail_stream_stride, char *have_d,
                                  long long have_stream_stride)
{
  AWM_ENTER (ctx);
  return sliding_rows_body (ctx, "awm_debug_sync_db_sliding_rows_d", pcm_d, false, n_frames, n_channels, base_d, count_d, n_streams, count0, rows_per_plane,
                            row_perm_d, band_pos_d, first, last, stream_range_d, range_index_d, range_div, tables_per_slice, ld, out_d, tail_d,
                            tail_stream_stride, have_d, have_stream_stride);
}

/* The refusals that every entry point for a whole stream of 16-bit PCM adds to its float twin's: AWM_ERR_ARG, nothing enqueued.  The odd
 * address and the missing stream first; then the form of K4s, of which only the default has a 16-bit instantiation */
static int
check_stream_s16 (const char *who, const int16_t *pcm_d, size_t n_frames, int n_channels)
{
  const char *bad = nullptr;
  if (reinterpret_cast<uintptr_t> (pcm_d) & 1)
    bad = "pcm_d is not 2-byte aligned";
  else if (!pcm_d && n_frames)
    bad = "pcm_d is null";
  else if (n_channels < 1)
    bad = "n_channels < 1";
  else if (!awmk::sliding_s16_form_ok())
    bad = "16-bit streams run the default form of the refinement only (awm_debug_set_refine_form)";
  if (!bad)
    return 0;
  set_error (std::string (who) + ": " + bad);
  return AWM_ERR_ARG;
}

static DeviceWav
make_wav_s16 (const int16_t *pcm_d, size_t n_frames, int n_channels, int rate = Params::mark_sample_rate)
{
  DeviceWav w = make_wav_rate (nullptr, n_frames, n_channels, rate);
  w.pcm16 = n_frames ? pcm_d : nullptr;
  return w;
}

int
awm_debug_sync_db_sliding_rows_s16_d (awm_ctx *ctx, const int16_t *pcm_d, size_t n_frames, int n_channels, const long long *base_d, const int *count_d,
                                      size_t n_streams, int count0, int rows_per_plane, const int *row_perm_d, const unsigned char *band_pos_d,
                                      long long first, long long last, const long long *stream_range_d, const int *range_index_d, int range_div,
                                      int tables_per_slice, int ld, float *out_d, float *tail_d, long long tail_stream_stride, char *have_d,
                                      long long have_stream_stride)
{
  AWM_ENTER (ctx);
  if (int rc = check_stream_s16 ("awm_debug_sync_db_sliding_rows_s16_d", pcm_d, n_frames, n_channels))
    return rc;
  return sliding_rows_body (ctx, "awm_debug_sync_db_sliding_rows_s16_d", pcm_d, true, n_frames, n_channels, base_d, count_d, n_streams, count0,
                            rows_per_plane, row_perm_d, band_pos_d, first, last, stream_range_d, range_index_d, range_div, tables_per_slice, ld, out_d,
                            tail_d, tail_stream_stride, have_d, have_stream_stride);
}

/* the body of awm_sync_fft_d and of its 16-bit twin */
static int
sync_fft_body (awm_ctx *ctx, const char *who, const DeviceWav& wav, size_t index, size_t frame_count,
               const char *want_frames, size_t first, size_t last, float *db_out_d, char *have_out_d)
{
  const size_t n_frames = wav.n_frames;
  const int n_channels = wav.n_channels;
  auto launch_db = [&] (hipStream_t s, const awmk::SyncDbArgs& args) {
    return wav.s16() ? awmk::launch_sync_db_s16 (s, ctx->tabs, args) : awmk::launch_sync_db (s, ctx->tabs, args);
  };
  if (n_frames < index + frame_count * Params::frame_size)
    {
      set_error (std::string (who) + ": read past end");       // the reference returns empty vectors here
      return AWM_ERR_ARG;
    }
  if (!frame_count)
    return 0;
  // band-major scratch, then transposed into the reference's [frame][81] layout by a strided copy
  const long long ld = (long long) ((frame_count + 63) & ~size_t (63));
  if (int rc = ctx->ws_db.reserve (size_t (ld) * Params::n_bands * sizeof (float))) return rc;
  if (int rc = ctx->ws_have.reserve (ld)) return rc;
  hipStream_t st = ctx->stream;
  std::vector<long long> bases;
  std::vector<int> counts;
  awmk::SyncDbArgs da {};
  da.pcm = wav.pcm_arg();
  da.n_frames = (long long) n_frames;
  da.n_channels = n_channels;
  da.per_channel = 0;
  da.hop = Params::frame_size;
  da.out = ctx->ws_db.as<float>();
  da.ld = ld;
  da.have = ctx->ws_have.as<char>();
  da.first = (long long) first;
  da.last = (long long) last;
  da.tile_frames = 32;
  AWM_HIP_CHECK (hipMemsetAsync (ctx->ws_db.ptr, 0, size_t (ld) * Params::n_bands * sizeof (float), st));
  AWM_HIP_CHECK (hipMemsetAsync (ctx->ws_have.ptr, 0, ld, st));
  if (!want_frames)
    {
      da.base0 = (long long) index;
      da.base_stride = 0;
      da.count0 = int (frame_count);
      da.n_streams = 1;
      da.out_stream_stride = 0;
      da.have_stream_stride = 0;
      AWM_HIP_CHECK (launch_db (st, da));
    }
  else
    {
      // one single-frame stream per wanted frame, written at its own column
      for (size_t f = 0; f < frame_count; f++)
        if (want_frames[f])
          bases.push_back ((long long) (index + f * Params::frame_size));
      if (!bases.empty())
        {
          // process wanted frames one launch per contiguous run to keep column addressing simple
          size_t f = 0;
          while (f < frame_count)
            {
              if (!want_frames[f])
                {
                  f++;
                  continue;
                }
              size_t g = f;
              while (g < frame_count && want_frames[g])
                g++;
              awmk::SyncDbArgs run = da;
              run.base0 = (long long) (index + f * Params::frame_size);
              run.base_stride = 0;
              run.count0 = int (g - f);
              run.n_streams = 1;
              run.out = da.out + f;
              run.have = da.have + f;
              run.out_stream_stride = 0;
              run.have_stream_stride = 0;
              AWM_HIP_CHECK (launch_db (st, run));
              f = g;
            }
        }
    }
  // transpose [81][ld] -> [frame_count][81]
  AWM_HIP_CHECK (hipMemcpy2DAsync (have_out_d, 1, ctx->ws_have.ptr, 1, 1, frame_count, hipMemcpyDeviceToDevice, st));
  for (int b = 0; b < Params::n_bands; b++)
    AWM_HIP_CHECK (hipMemcpy2DAsync (db_out_d + b, Params::n_bands * sizeof (float), ctx->ws_db.as<float>() + (long long) b * ld,
                                     sizeof (float), sizeof (float), frame_count, hipMemcpyDeviceToDevice, st));
  return 0;
}

int
awm_sync_fft_d (awm_ctx *ctx, const float *pcm_d, size_t n_frames, int n_channels, size_t index, size_t frame_count,
                const char *want_frames, size_t first, size_t last, float *db_out_d, char *have_out_d)
{
  AWM_ENTER (ctx);
  return sync_fft_body (ctx, "awm_sync_fft_d", make_wav (pcm_d, n_frames, n_channels), index, frame_count, want_frames, first, last, db_out_d, have_out_d);
}

int
awm_sync_fft_s16_d (awm_ctx *ctx, const int16_t *pcm_d, size_t n_frames, int n_channels, size_t index, size_t frame_count,
                    const char *want_frames, size_t first, size_t last, float *db_out_d, char *have_out_d)
{
  AWM_ENTER (ctx);
  if (int rc = check_stream_s16 ("awm_sync_fft_s16_d", pcm_d, n_frames, n_channels))
    return rc;
  return sync_fft_body (ctx, "awm_sync_fft_s16_d", make_wav_s16 (pcm_d, n_frames, n_channels), index, frame_count, want_frames, first, last, db_out_d,
                        have_out_d);
}

static int
sync_search_body (awm_ctx *ctx, const uint8_t key[16], const DeviceWav& wav, int clip_mode, size_t max_out, uint64_t *index, double *quality,
                  int *block_type)
{
  SyncFinder sf (ctx);
  std::vector<SyncFinder::Score> scores;
  if (int rc = sf.search (capi_key (key), wav, clip_mode ? SyncFinder::Mode::CLIP : SyncFinder::Mode::BLOCK, scores))
    return rc;
  for (size_t i = 0; i < scores.size() && i < max_out; i++)
    {
      index[i] = scores[i].index;
      quality[i] = scores[i].quality;
      block_type[i] = int (scores[i].block_type);
    }
  return int (scores.size());
}

int
awm_sync_search_s16_d (awm_ctx *ctx, const uint8_t key[16], const int16_t *pcm_d, size_t n_frames, int n_channels, int clip_mode,
                       size_t max_out, uint64_t *index, double *quality, int *block_type)
{
  AWM_ENTER (ctx);
  if (int rc = check_stream_s16 ("awm_sync_search_s16_d", pcm_d, n_frames, n_channels))
    return rc;
  return sync_search_body (ctx, key, make_wav_s16 (pcm_d, n_frames, n_channels), clip_mode, max_out, index, quality, block_type);
}

int
awm_sync_search_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int clip_mode,
                   size_t max_out, uint64_t *index, double *quality, int *block_type)
{
  AWM_ENTER (ctx);
  return sync_search_body (ctx, key, make_wav (pcm_d, n_frames, n_channels), clip_mode, max_out, index, quality, block_type);
}

long
awm_search_approx_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int clip_mode,
                     size_t max_out, uint64_t *index, double *raw_quality, double *local_mean)
{
  AWM_ENTER (ctx);
  KeyTables *kt = ctx->get_key_tables (capi_key (key));
  if (!kt)
    return AWM_ERR_HIP;
  SyncFinder sf (ctx);
  std::vector<SyncFinder::SearchScore> scores;
  const DeviceWav wav = make_wav (pcm_d, n_frames, n_channels);
  if (int rc = sf.prepare (wav, clip_mode ? SyncFinder::Mode::CLIP : SyncFinder::Mode::BLOCK))
    return rc;
  if (int rc = sf.search_approx (kt, wav, clip_mode ? SyncFinder::Mode::CLIP : SyncFinder::Mode::BLOCK, scores))
    return rc;
  for (size_t i = 0; i < scores.size() && i < max_out; i++)
    {
      index[i] = scores[i].index;
      raw_quality[i] = scores[i].raw_quality;
      local_mean[i] = scores[i].local_mean;
    }
  return long (scores.size());
}

static int
block_soft_bits_body (awm_ctx *ctx, const uint8_t key[16], const DeviceWav& wav, const uint64_t *index, size_t n_blocks, float *out, int *ok)
{
  KeyTables *kt = ctx->get_key_tables (capi_key (key));
  if (!kt)
    return AWM_ERR_HIP;
  std::vector<size_t> idx (index, index + n_blocks);
  std::vector<std::vector<float>> raw;
  std::vector<char> okv;
  if (int rc = block_soft_bits (ctx, kt, wav, idx, raw, okv))
    return rc;
  const size_t n_bits = mark_data_frame_count() / params().frames_per_bit;
  for (size_t i = 0; i < n_blocks; i++)
    {
      ok[i] = okv[i];
      if (okv[i])
        std::copy (raw[i].begin(), raw[i].end(), out + i * n_bits);
      else
        std::fill (out + i * n_bits, out + (i + 1) * n_bits, 0.f);
    }
  return 0;
}

int
awm_block_soft_bits_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels,
                       const uint64_t *index, size_t n_blocks, float *out, int *ok)
{
  AWM_ENTER (ctx);
  return block_soft_bits_body (ctx, key, make_wav (pcm_d, n_frames, n_channels), index, n_blocks, out, ok);
}

int
awm_block_soft_bits_s16_d (awm_ctx *ctx, const uint8_t key[16], const int16_t *pcm_d, size_t n_frames, int n_channels,
                           const uint64_t *index, size_t n_blocks, float *out, int *ok)
{
  AWM_ENTER (ctx);
  if (int rc = check_stream_s16 ("awm_block_soft_bits_s16_d", pcm_d, n_frames, n_channels))
    return rc;
  return block_soft_bits_body (ctx, key, make_wav_s16 (pcm_d, n_frames, n_channels), index, n_blocks, out, ok);
}

/* ---- debug views of the block decoder's dB pass and soft bits (K4b, K7): tests only ---- */
namespace {

constexpr size_t DEBUG_BLOCKS_MAX = 64;
constexpr long long DEBUG_RANGE_MAX = 1LL << 40;

/* the ranges of padded slices as the kernels may be given them: [n_slices][2] on the device, first < 0 (nothing but silence) or
 * 0 <= first <= last <= max_value; one synchronisation */
int
debug_check_ranges (awm_ctx *ctx, const long long *slice_range_d, size_t n_slices, long long max_value, const char *&bad)
{
  std::vector<long long> r (2 * n_slices);
  AWM_HIP_CHECK (hipMemcpyAsync (r.data(), slice_range_d, r.size() * sizeof (long long), hipMemcpyDeviceToHost, ctx->stream));
  AWM_HIP_CHECK (hipStreamSynchronize (ctx->stream));
  for (size_t s = 0; s < n_slices && !bad; s++)
    if (r[2 * s] >= 0 && (r[2 * s] > r[2 * s + 1] || r[2 * s + 1] > max_value))
      bad = "a slice's range is not first < 0 or 0 <= first <= last <= the values there are";
  return 0;
}

}

int
awm_debug_block_plane_ld (awm_ctx *ctx)
{
  AWM_ENTER (ctx);
  return int (block_plane_ld());
}

int
awm_debug_block_db_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, const uint64_t *index,
                      size_t n_blocks, uint32_t fill, const long long *slice_range_d, size_t n_slices, size_t slice_frames,
                      float *planes_out_d, size_t planes_values, float *soft_out, int *slot_out)
{
  AWM_ENTER (ctx);
  const size_t block_values = size_t (std::max (n_channels, 0)) * Params::n_bands * size_t (block_plane_ld());
  const size_t block_len = mark_block_frame_count() * Params::frame_size;
  const char *bad = nullptr;
  if (!pcm_d || !index || !planes_out_d || !soft_out || !slot_out)
    bad = "null pointer";
  else if (n_channels < 1 || n_channels > 3)
    bad = "1, 2 or 3 channels";
  else if (n_blocks < 1 || n_blocks > DEBUG_BLOCKS_MAX)
    bad = "1 .. 64 blocks";
  else if (n_frames > size_t (DEBUG_RANGE_MAX))
    bad = "too many frames";
  else if (planes_values / block_values < n_blocks)
    bad = "planes_out_d holds fewer than n_blocks blocks";
  else if ((slice_range_d != nullptr) != (slice_frames != 0) || (slice_range_d != nullptr) != (n_slices != 0))
    bad = "slice_range_d, n_slices and slice_frames go together";
  else if (slice_range_d && (slice_frames > n_frames || n_slices > n_frames / slice_frames))
    bad = "the slices do not fit into the samples";
  if (!bad && slice_range_d)
    for (size_t i = 0; i < n_blocks && !bad; i++)
      if (index[i] <= n_frames && n_frames - index[i] >= block_len && index[i] / slice_frames >= n_slices)      // (an accepted block)
        bad = "a block starts behind the last slice";
  if (!bad && slice_range_d)
    if (int rc = debug_check_ranges (ctx, slice_range_d, n_slices, (long long) (n_frames * n_channels), bad))
      return rc;
  if (bad)
    {
      set_error (std::string ("awm_debug_block_db_d: ") + bad);
      return AWM_ERR_ARG;
    }
  KeyTables *kt = ctx->get_key_tables (capi_key (key));
  if (!kt)
    return AWM_ERR_HIP;
  const size_t n_bits = mark_data_frame_count() / params().frames_per_bit;
  const std::vector<size_t> idx (index, index + n_blocks);
  std::vector<int> slot_of;
  std::vector<char> ok;
  const BlockDbView view { fill, planes_out_d };
  if (int rc = block_soft_bits_dev (ctx, ctx, kt, make_wav (pcm_d, n_frames, n_channels), idx, slot_of, ok, slice_range_d, slice_frames, &view))
    return rc;
  size_t n_slots = 0;
  for (size_t i = 0; i < n_blocks; i++)
    {
      slot_out[i] = slot_of[i];
      n_slots = std::max (n_slots, size_t (slot_of[i] + 1));
    }
  if (n_slots)
    AWM_HIP_CHECK (hipMemcpyAsync (soft_out, ctx->ws_soft.ptr, n_slots * n_bits * sizeof (float), hipMemcpyDeviceToHost, ctx->stream));
  AWM_HIP_CHECK (stream_wait (ctx->stream));
  return 0;
}

int
awm_debug_soft_bits_planes_d (awm_ctx *ctx, const uint8_t key[16], const float *planes_d, size_t planes_values, size_t n_blocks, int n_channels,
                              const long long *block_base_d, const long long *slice_range_d, const int *range_index_d, size_t n_slices,
                              float *soft_out)
{
  AWM_ENTER (ctx);
  const size_t block_values = size_t (std::max (n_channels, 0)) * Params::n_bands * size_t (block_plane_ld());
  const bool ranges = slice_range_d != nullptr;
  const char *bad = nullptr;
  if (!planes_d || !soft_out)
    bad = "null pointer";
  else if (n_channels < 1 || n_channels > 3)
    bad = "1, 2 or 3 channels";
  else if (n_blocks < 1 || n_blocks > DEBUG_BLOCKS_MAX)
    bad = "1 .. 64 blocks";
  else if (planes_values / block_values < n_blocks)
    bad = "planes_d holds fewer than n_blocks blocks";
  else if ((block_base_d != nullptr) != ranges || (range_index_d != nullptr) != ranges || (n_slices != 0) != ranges)
    bad = "block_base_d, slice_range_d, range_index_d and n_slices go together";
  if (!bad && ranges)
    {
      std::vector<long long> base (n_blocks);
      std::vector<int> slice (n_blocks);
      AWM_HIP_CHECK (hipMemcpyAsync (base.data(), block_base_d, n_blocks * sizeof (long long), hipMemcpyDeviceToHost, ctx->stream));
      AWM_HIP_CHECK (hipMemcpyAsync (slice.data(), range_index_d, n_blocks * sizeof (int), hipMemcpyDeviceToHost, ctx->stream));
      if (int rc = debug_check_ranges (ctx, slice_range_d, n_slices, DEBUG_RANGE_MAX * n_channels, bad))
        return rc;
      for (size_t i = 0; i < n_blocks && !bad; i++)
        if (base[i] < 0 || base[i] > DEBUG_RANGE_MAX || slice[i] < 0 || size_t (slice[i]) >= n_slices)
          bad = "a block's base or slice is out of range";
    }
  if (bad)
    {
      set_error (std::string ("awm_debug_soft_bits_planes_d: ") + bad);
      return AWM_ERR_ARG;
    }
  KeyTables *kt = ctx->get_key_tables (capi_key (key));
  if (!kt)
    return AWM_ERR_HIP;
  const size_t n_bits = mark_data_frame_count() / params().frames_per_bit;
  if (int rc = ctx->ws_soft.reserve (n_blocks * n_bits * sizeof (float))) return rc;
  const awmk::SoftBitsArgs sb = block_soft_args (kt, n_channels, planes_d, n_blocks, ctx->ws_soft.as<float>(), block_base_d, range_index_d,
                                                 slice_range_d, ranges);
  AWM_HIP_CHECK (awmk::launch_soft_bits (ctx->stream, sb));
  AWM_HIP_CHECK (hipMemcpyAsync (soft_out, ctx->ws_soft.ptr, n_blocks * n_bits * sizeof (float), hipMemcpyDeviceToHost, ctx->stream));
  AWM_HIP_CHECK (stream_wait (ctx->stream));
  return 0;
}

int
awm_viterbi_decode (awm_ctx *ctx, int block_type, const float *soft, size_t coded_len, size_t n, int *bits_out, float *error_out)
{
  AWM_ENTER (ctx);
  if (block_type < 0 || block_type > 2)
    return AWM_ERR_ARG;
  std::vector<std::vector<float>> in (n);
  for (size_t i = 0; i < n; i++)
    in[i].assign (soft + i * coded_len, soft + (i + 1) * coded_len);
  std::vector<std::vector<int>> bits;
  std::vector<float> errors;
  if (int rc = viterbi_decode (ctx, ConvBlockType (block_type), in, bits, errors))
    return rc;
  for (size_t i = 0; i < n; i++)
    {
      std::copy (bits[i].begin(), bits[i].end(), bits_out + i * bits[i].size());
      error_out[i] = errors[i];
    }
  return 0;
}

int
awm_add_watermark_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const float *pcm_in_d, float *out_d,
                     size_t n_frames, int n_channels, int sample_rate)
{
  AWM_ENTER (ctx);
  if (n_channels >= 1 && add_buffers_overlap (pcm_in_d, out_d, n_frames * size_t (n_channels)))
    {
      set_error ("awm_add_watermark_d: the output overlaps the input");
      return AWM_ERR_ARG;
    }
  FrameModTable *fm = ctx->get_frame_mod (capi_key (key), payload_hex ? payload_hex : "");
  if (!fm)
    return AWM_ERR_ARG;
  if (sample_rate != Params::mark_sample_rate)
    return add_full_rate (ctx, pcm_in_d, out_d, n_frames, n_channels, fm->dev.as<int8_t>(), params().water_delta, !params().test_no_limiter, sample_rate);
  return add_full (ctx, pcm_in_d, out_d, n_frames, n_channels, fm->dev.as<int8_t>(), params().water_delta, !params().test_no_limiter);
}

/* One input, many payloads (include/awm_hip.h).  At 44.1 kHz the payloads go through K2m in tiles of ADD_MULTI_TILE outputs: a tile pass
 * reads the input once and transforms every frame forward once, whatever the number of its outputs; block maxima and limiter ramp are
 * per output.  At a rate with fixed-ratio tables both ways the stream is resampled to 44.1 kHz once, K2m writes the watermark signals of
 * a pass alone and they go up and into the outputs per pass (add_payloads_rate); every other rate, one payload and the debug toggles
 * loop over the single-payload path. */
extern "C" void awm_debug_set_add_payloads_fused (int on) { g_add_payloads_fused = on; }
extern "C" int  awm_debug_add_payloads_fused_in_use (void) { return g_add_payloads_fused_in_use; }
extern "C" int  awm_debug_add_payloads_tile (void) { return awmk::ADD_MULTI_TILE; }
static int g_add_payloads_rate_fused = 2, g_add_payloads_rate_fused_in_use = 0;
extern "C" void awm_debug_set_add_payloads_rate_fused (int mode) { g_add_payloads_rate_fused = mode < 0 ? 0 : mode > 2 ? 2 : mode; }
extern "C" int  awm_debug_add_payloads_rate_fused_in_use (void) { return g_add_payloads_rate_fused_in_use; }

/* awm_add_watermark_payloads_d at another sample rate: add_full_rate's stages with everything that does not depend
 * on the payload done once.  The stream goes down to 44.1 kHz once for the call (x44; F, n44 and last44 are add_full_rate's); per balanced
 * pass of at most ADD_MULTI_TILE payloads K2m (delta_only) reads x44 once and writes the pass's watermark signals, which K10m takes up to
 * the rate and adds to the stream in one kernel (stereo 44.1 -> 48 kHz, every pointer 8-byte aligned: path 2) or K10 and K11 once per
 * output (everything else: path 1); then the limiter per output.  Every output is computed by add_full_rate's own arithmetic, value for
 * value, and block maxima are maxima: the outputs are the loop's bit for bit.
 * Workspaces: x44 and min (P, ADD_MULTI_TILE) watermark signals of n44 C floats each, path 1 also one signal at the rate -- 60 min of
 * stereo at 48 kHz with P >= 4: 5 x 1.27 GB = 6.4 GB for path 2 (the loop: 2 x 1.27 + 1.38 = 3.9 GB).  *taken = false, nothing enqueued:
 * a reservation failed (what had been reserved is freed again) and the caller runs the loop. */
static int
add_payloads_rate (awm_ctx *ctx, const Key& k, const char *const *payload_hex, size_t n_payloads, const float *pcm_in_d, float *const *out_d,
                   size_t n_frames, int C, double water_delta, int use_limiter, int rate, const RateConverter& down, const RateConverter& up,
                   bool *taken)
{
  hipStream_t st = ctx->stream;
  const size_t last44 = up.window_start (n_frames - 1) + size_t (up.hl()) + 1;
  const size_t F = last44 / Params::frame_size + 1;              // watermark frames 0 .. F - 1 are needed
  const size_t n44 = (F + 1) * Params::frame_size;               // frame F's delta completes frame F - 1
  const size_t n_ws = std::min<size_t> (n_payloads, size_t (awmk::ADD_MULTI_TILE)), ws_values = n44 * size_t (C);
  const int lim_block = int (size_t (rate) * size_t (Params::limiter_block_size_ms) / 1000);
  const size_t n_blocks = n_frames / lim_block + 2;
  const ResampleTable& ut = *up.fixed;
  awmk::ResampleMixArgs ma {};
  ma.orig = pcm_in_d;
  ma.n_in = (long long) (F * Params::frame_size);                // only frames 0 .. F - 1 of a signal are complete (add_full_rate)
  ma.n_channels = C;
  ma.ctab = ut.ctab.as<float>();
  ma.hl = ut.hl;
  ma.np = ut.np;
  ma.step = ut.step;
  ma.n_out = (long long) n_frames;
  ma.n_blocks = (long long) n_blocks;
  ma.limiter_block = lim_block;
  ma.n = 1;
  bool mixed = g_add_payloads_rate_fused == 2;
  for (size_t p = 0; mixed && p < n_payloads; p++)
    {
      ma.o[0].wm44 = pcm_in_d;                                   // (the workspaces are aligned; the launcher checks them again)
      ma.o[0].out = out_d[p];
      mixed = awmk::resample_mix_multi_takes (ma);
    }
  *taken = false;
  if (ctx->ws_rate_a.reserve (ws_values * sizeof (float)) || ctx->ws_rate_b.reserve (n_ws * ws_values * sizeof (float))
      || (!mixed && ctx->ws_rate_c.reserve (n_frames * C * sizeof (float))))
    {
      ctx->ws_rate_a.release();
      ctx->ws_rate_b.release();
      ctx->ws_rate_c.release();
      return 0;
    }
  float *block_max = nullptr;
  size_t tab_entries = 0;
  if (use_limiter)
    {
      if (int rc = ctx->ws_block_max.reserve (n_payloads * n_blocks * sizeof (float))) return rc;
      tab_entries = awmk::limiter_tab_entries ((long long) n_frames, 0, lim_block);
      if (int rc = ctx->ws_limit_tab.reserve ((tab_entries + 1) * sizeof (float2))) return rc;
      block_max = ctx->ws_block_max.as<float>();
      unsigned int bits;
      std::memcpy (&bits, &LIMITER_CEILING, sizeof (bits));
      AWM_HIP_CHECK (awmk::launch_fill_u32 (st, reinterpret_cast<unsigned int *> (block_max), bits, n_payloads * n_blocks));
    }
  *taken = true;
  float *x44 = ctx->ws_rate_a.as<float>(), *wm44 = ctx->ws_rate_b.as<float>(), *wm = ctx->ws_rate_c.as<float>();
  if (int rc = resample_device (ctx, down, pcm_in_d, n_frames, C, x44, n44)) return rc;
  awmk::AddMixMultiArgs a {};
  a.pcm_in = x44;
  a.n_frames = (long long) n44;
  a.n_channels = C;
  fill_add_mix_common (a, water_delta);
  a.frames_per_span = frames_per_span (ctx, (long long) (F + 1), awmk::add_mix_multi_waves_per_simd());
  a.delta_only = 1;
  auto maxima = [&] (size_t p) { return use_limiter ? reinterpret_cast<unsigned int *> (block_max + p * n_blocks) : nullptr; };
  const int rc = add_mix_multi_passes (ctx, st, a, n_payloads,
    [&] (size_t p, awmk::AddMixOut& o) {
      FrameModTable *fm = ctx->get_frame_mod (k, payload_hex[p]);
      if (!fm)
        return false;
      o.out = wm44 + size_t (&o - a.o) * ws_values;             // the pass's i-th signal
      o.frame_mod = fm->dev.as<int8_t>();
      o.block_max = nullptr;
      return true;
    },
    [&] () { AWM_HIP_CHECK (awmk::launch_add_mix_multi (st, ctx->tabs, a)); return 0; },
    [&] (size_t p0, size_t n) {
      if (mixed)
        {
          ma.n = int (n);
          for (size_t i = 0; i < size_t (awmk::ADD_MULTI_TILE); i++)
            ma.o[i] = i < n ? awmk::ResampleMixOut { wm44 + i * ws_values, out_d[p0 + i], maxima (p0 + i) } : awmk::ResampleMixOut {};
          // the stream once, every signal and every output once
          ProfScope ps (ctx, PROF_RESAMPLE_MIX, (double (n_frames) * (1 + n) + double (ma.n_in) * n) * C * 4.0, st);
          AWM_HIP_CHECK (awmk::launch_resample_mix_multi (st, ma));
        }
      else
        for (size_t i = 0; i < n; i++)
          {
            if (int r = resample_device (ctx, up, wm44 + i * ws_values, F * Params::frame_size, C, wm, n_frames)) return r;
            AWM_HIP_CHECK (awmk::launch_mix_max (st, pcm_in_d, wm, out_d[p0 + i], (long long) n_frames, C, maxima (p0 + i), (long long) n_blocks, lim_block));
          }
      for (size_t p = p0; use_limiter && p < p0 + n; p++)
        {
          ProfScope ps (ctx, PROF_LIMITER, double (n_frames) * C * 8.0, st);
          // (the outputs share the ramp table: the passes run in stream order, each rebuilds the entries)
          AWM_HIP_CHECK (awmk::launch_limiter (st, out_d[p], (long long) n_frames, C, 0, block_max + p * n_blocks, 0, (long long) n_blocks,
                                               lim_block, LIMITER_CEILING, ctx->ws_limit_tab.as<float2>(), tab_entries));
        }
      return 0;
    });
  if (rc)
    return rc;
  g_add_payloads_rate_fused_in_use = mixed ? 2 : 1;
  return 0;
}

int
awm_add_watermark_payloads_d (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads,
                              const float *pcm_in_d, float *const *out_d, size_t n_frames, int n_channels, int sample_rate)
{
  AWM_ENTER (ctx);
  g_add_payloads_fused_in_use = 0;
  g_add_payloads_rate_fused_in_use = 0;
  if (!n_payloads || !n_frames)
    return 0;
  if (!key || !payload_hex || !pcm_in_d || !out_d || n_channels < 1)
    {
      set_error ("awm_add_watermark_payloads_d: bad argument");
      return AWM_ERR_ARG;
    }
  if (ctx->snr_on)
    {
      set_error ("awm_add_watermark_payloads_d: not available while the SNR meter is armed (awm_ctx_snr_begin)");
      return AWM_ERR_ARG;
    }
  // everything is checked before anything is enqueued: the input is read for every output, so no output may overlap it or another one
  const size_t n_values = n_frames * size_t (n_channels);
  auto overlap = [n_values] (const float *a, const float *b) { return a < b + n_values && b < a + n_values; };
  for (size_t p = 0; p < n_payloads; p++)
    {
      if (!payload_hex[p] || !out_d[p])
        {
          set_error (string_printf ("awm_add_watermark_payloads_d: null pointer at index %zu", p));
          return AWM_ERR_ARG;
        }
      if (parse_payload (payload_hex[p]).empty())
        {
          set_error (string_printf ("awm_add_watermark_payloads_d: cannot parse payload '%s' at index %zu", payload_hex[p], p));
          return AWM_ERR_ARG;
        }
      if (overlap (out_d[p], pcm_in_d))
        {
          set_error (string_printf ("awm_add_watermark_payloads_d: output %zu overlaps the input", p));
          return AWM_ERR_ARG;
        }
      for (size_t q = 0; q < p; q++)
        if (overlap (out_d[p], out_d[q]))
          {
            set_error (string_printf ("awm_add_watermark_payloads_d: outputs %zu and %zu overlap", q, p));
            return AWM_ERR_ARG;
          }
    }
  const Key k = capi_key (key);
  const double water_delta = params().water_delta;
  const int use_limiter = !params().test_no_limiter;
  if (n_payloads > 1 && g_add_payloads_fused && g_add_payloads_rate_fused && sample_rate != Params::mark_sample_rate && sample_rate > 0)
    {
      // rates that only the VResampler takes have no table one way or the other: the loop
      RateConverter down, up;
      down.fixed = ctx->get_resample_table (sample_rate, Params::mark_sample_rate);
      up.fixed = down.fixed ? ctx->get_resample_table (Params::mark_sample_rate, sample_rate) : nullptr;
      if (down.fixed && up.fixed)
        {
          bool taken = false;
          const int rc = add_payloads_rate (ctx, k, payload_hex, n_payloads, pcm_in_d, out_d, n_frames, n_channels, water_delta, use_limiter,
                                            sample_rate, down, up, &taken);
          if (rc || taken)
            return rc;
        }
    }
  if (n_payloads == 1 || !g_add_payloads_fused || sample_rate != Params::mark_sample_rate)
    {
      for (size_t p = 0; p < n_payloads; p++)
        {
          FrameModTable *fm = ctx->get_frame_mod (k, payload_hex[p]);
          if (!fm)
            return AWM_ERR_ARG;
          const int rc = sample_rate != Params::mark_sample_rate
                       ? add_full_rate (ctx, pcm_in_d, out_d[p], n_frames, n_channels, fm->dev.as<int8_t>(), water_delta, use_limiter, sample_rate)
                       : add_full (ctx, pcm_in_d, out_d[p], n_frames, n_channels, fm->dev.as<int8_t>(), water_delta, use_limiter);
          if (rc)
            return rc;
        }
      return 0;
    }

  hipStream_t st = ctx->stream;
  const size_t n_blocks = n_frames / LIMITER_BLOCK + 2;
  float *block_max = nullptr;
  size_t tab_entries = 0;
  if (use_limiter)
    {
      if (int rc = ctx->ws_block_max.reserve (n_payloads * n_blocks * sizeof (float))) return rc;
      block_max = ctx->ws_block_max.as<float>();
      unsigned int bits;
      std::memcpy (&bits, &LIMITER_CEILING, sizeof (bits));
      AWM_HIP_CHECK (awmk::launch_fill_u32 (st, reinterpret_cast<unsigned int *> (block_max), bits, n_payloads * n_blocks));
      tab_entries = awmk::limiter_tab_entries ((long long) n_frames, 0, LIMITER_BLOCK);
      if (int rc = ctx->ws_limit_tab.reserve ((tab_entries + 1) * sizeof (float2))) return rc;
    }
  awmk::AddMixMultiArgs a {};
  a.pcm_in = pcm_in_d;
  a.n_frames = (long long) n_frames;
  a.n_channels = n_channels;
  fill_add_mix_common (a, water_delta);
  a.n_blocks = (long long) n_blocks;
  a.frames_per_span = frames_per_span (ctx, (long long) (n_frames + 1023) / 1024, awmk::add_mix_multi_waves_per_simd());
  const int rc = add_mix_multi_passes (ctx, st, a, n_payloads,
    [&] (size_t p, awmk::AddMixOut& o) {
      // (the cache holds far more than a tile, and drains the device before it drops one)
      FrameModTable *fm = ctx->get_frame_mod (k, payload_hex[p]);
      if (!fm)
        return false;
      o.out = out_d[p];
      o.frame_mod = fm->dev.as<int8_t>();
      o.block_max = use_limiter ? reinterpret_cast<unsigned int *> (block_max + p * n_blocks) : nullptr;
      return true;
    },
    [&] () { AWM_HIP_CHECK (awmk::launch_add_mix_multi (st, ctx->tabs, a)); return 0; },
    [&] (size_t p0, size_t n) {
      for (size_t p = p0; use_limiter && p < p0 + n; p++)
        {
          ProfScope ps (ctx, PROF_LIMITER, double (n_frames) * n_channels * 8.0, st);
          // (the outputs share the ramp table: the passes run in stream order, each rebuilds the entries)
          AWM_HIP_CHECK (awmk::launch_limiter (st, out_d[p], (long long) n_frames, n_channels, 0, block_max + p * n_blocks, 0, (long long) n_blocks,
                                               LIMITER_BLOCK, LIMITER_CEILING, ctx->ws_limit_tab.as<float2>(), tab_entries));
        }
      return 0;
    });
  if (rc)
    return rc;
  g_add_payloads_fused_in_use = 1;
  return 0;
}

/* The P-output twin of add_mix_impl: one span of a stream, a table (on the device), an output and -- with the limiter -- an array of block
 * maxima per payload.  Passes of at most ADD_MULTI_TILE outputs through K2m's span form, balanced like the whole-stream entry; with the
 * toggle off (or one payload) a loop over K2.  Nothing is checked here. */
static int
add_mix_payloads_impl (awm_ctx *ctx, const float *pcm_in_d, float *const *out_d, size_t n_payloads, size_t n_frames, int n_channels,
                       const int8_t *const *frame_mod_dev, double water_delta, size_t first_frame, const float *halo_before_d,
                       const float *halo_after_d, float *const *block_max_d, size_t first_block, size_t n_blocks, int delta_only)
{
  g_add_payloads_fused_in_use = 0;
  if (n_payloads == 1 || !g_add_payloads_fused)
    {
      for (size_t p = 0; p < n_payloads; p++)
        if (int rc = add_mix_impl (ctx, pcm_in_d, out_d[p], n_frames, n_channels, frame_mod_dev[p], water_delta, first_frame, halo_before_d,
                                   halo_after_d, block_max_d ? block_max_d[p] : nullptr, first_block, n_blocks, nullptr, delta_only))
          return rc;
      return 0;
    }
  hipStream_t st = ctx->stream;
  awmk::AddMixMultiArgs a {};
  a.pcm_in = pcm_in_d;
  a.n_frames = (long long) n_frames;
  a.n_channels = n_channels;
  fill_add_mix_common (a, water_delta);
  a.n_blocks = (long long) n_blocks;
  a.frames_per_span = frames_per_span (ctx, (long long) (n_frames + 1023) / 1024, awmk::add_mix_multi_span_waves_per_simd());
  a.delta_only = delta_only;
  awmk::AddMixSpan sp {};
  sp.first_frame = (long long) first_frame;
  sp.halo_before = halo_before_d;
  sp.halo_after = halo_after_d;
  sp.first_block = (long long) first_block;
  const int rc = add_mix_multi_passes (ctx, st, a, n_payloads,
    [&] (size_t p, awmk::AddMixOut& o) {
      o.out = out_d[p];
      o.frame_mod = frame_mod_dev[p];
      o.block_max = block_max_d ? reinterpret_cast<unsigned int *> (block_max_d[p]) : nullptr;
      return true;
    },
    [&] () { AWM_HIP_CHECK (awmk::launch_add_mix_multi_span (st, ctx->tabs, a, sp)); return 0; },
    [] (size_t, size_t) { return 0; });
  if (rc)
    return rc;
  g_add_payloads_fused_in_use = 1;
  return 0;
}

int
awm_add_mix_payloads_d (awm_ctx *ctx, const float *pcm_in_d, float *const *out_d, size_t n_payloads, size_t n_frames, int n_channels,
                        const int8_t *const *frame_mod, double water_delta, size_t first_frame, const float *halo_before_d,
                        const float *halo_after_d, float *const *block_max_d, size_t first_block, size_t n_blocks)
{
  AWM_ENTER (ctx);
  g_add_payloads_fused_in_use = 0;
  if (!n_payloads || !pcm_in_d || !out_d || !frame_mod || n_channels < 1)
    {
      set_error (n_payloads ? "awm_add_mix_payloads_d: bad argument" : "awm_add_mix_payloads_d: no payloads");
      return AWM_ERR_ARG;
    }
  if (ctx->snr_on && n_payloads > 1)
    {
      set_error ("awm_add_mix_payloads_d: not available while the SNR meter is armed (awm_ctx_snr_begin)");
      return AWM_ERR_ARG;
    }
  // everything is checked before anything is enqueued: the input and the halos are read for every output
  const size_t n_values = n_frames * size_t (n_channels), halo_values = size_t (Params::frame_size) * n_channels;
  auto overlap = [] (const float *a, size_t na, const float *b, size_t nb) { return a && b && a < b + nb && b < a + na; };
  for (size_t p = 0; p < n_payloads; p++)
    {
      if (!out_d[p] || !frame_mod[p] || (block_max_d && !block_max_d[p]))
        {
          set_error (string_printf ("awm_add_mix_payloads_d: null pointer at index %zu", p));
          return AWM_ERR_ARG;
        }
      if (overlap (out_d[p], n_values, pcm_in_d, n_values))
        {
          set_error (string_printf ("awm_add_mix_payloads_d: output %zu overlaps the input", p));
          return AWM_ERR_ARG;
        }
      if (overlap (out_d[p], n_values, halo_before_d, halo_values) || overlap (out_d[p], n_values, halo_after_d, halo_values))
        {
          set_error (string_printf ("awm_add_mix_payloads_d: output %zu overlaps a halo", p));
          return AWM_ERR_ARG;
        }
      for (size_t q = 0; q < p; q++)
        if (overlap (out_d[p], n_values, out_d[q], n_values))
          {
            set_error (string_printf ("awm_add_mix_payloads_d: outputs %zu and %zu overlap", q, p));
            return AWM_ERR_ARG;
          }
    }
  if (!n_frames)
    return 0;
  // the tables of all payloads side by side in the context's workspace
  const size_t table_bytes = 2 * mark_block_frame_count() * Params::n_bands;
  if (int rc = ctx->ws_misc.reserve (n_payloads * table_bytes)) return rc;
  std::vector<const int8_t *> tables (n_payloads);
  for (size_t p = 0; p < n_payloads; p++)
    {
      tables[p] = ctx->ws_misc.as<int8_t>() + p * table_bytes;
      AWM_HIP_CHECK (hipMemcpyAsync (ctx->ws_misc.as<int8_t>() + p * table_bytes, frame_mod[p], table_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
  return add_mix_payloads_impl (ctx, pcm_in_d, out_d, n_payloads, n_frames, n_channels, tables.data(), water_delta, first_frame, halo_before_d,
                                halo_after_d, block_max_d, first_block, n_blocks);
}

/* add_watermark followed by get_watermark of its output ("watermark, then verify") as ONE call: the library owns the order of the two
 * halves, so `get` may start chunk c as soon as the limiter has passed the chunk's last sample -- its first dB kernel (bound by FP32
 * issue) runs beside the limiter passes of the later ranges (bound by HBM) -- instead of behind the whole `add`, which is all that two
 * separate calls on the caller's stream can promise.  PCM and pattern list are those of the two calls (tests). */
int
awm_add_get_watermark_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const float *pcm_in_d, float *out_d,
                         size_t n_frames, int n_channels, int sample_rate, size_t max_out, awm_pattern *out)
{
  AWM_ENTER (ctx);
  if (max_out && !out)
    {
      set_error ("awm_add_get_watermark_d: bad argument");
      return AWM_ERR_ARG;
    }
  FrameModTable *fm = ctx->get_frame_mod (capi_key (key), payload_hex ? payload_hex : "");
  if (!fm)
    return AWM_ERR_ARG;
  int rc;
  const bool hand_over = sample_rate == Params::mark_sample_rate && pcm_in_d != out_d && !g_add_slab_mb && n_frames > 0;
  if (sample_rate != Params::mark_sample_rate)
    rc = add_full_rate (ctx, pcm_in_d, out_d, n_frames, n_channels, fm->dev.as<int8_t>(), params().water_delta, !params().test_no_limiter, sample_rate);
  else
    rc = add_full (ctx, pcm_in_d, out_d, n_frames, n_channels, fm->dev.as<int8_t>(), params().water_delta, !params().test_no_limiter, nullptr,
                   hand_over ? &ctx->ready : nullptr);
  if (rc)
    {
      ctx->ready.disarm();
      return rc;
    }
  ResultSet rs;
  if (sample_rate != Params::mark_sample_rate)
    {
      // the reference's loader resamples to the watermark rate before anything else (wavchunkloader.cc:70-71)
      const size_t n44 = awm_resample_frames (ctx, n_frames, sample_rate, Params::mark_sample_rate);
      if (n_frames && !n44)
        return AWM_ERR_ARG;
      if (int r = ctx->ws_rate_c.reserve (std::max<size_t> (1, n44 * n_channels * sizeof (float)))) return r;
      if (int r = awm_resample_d (ctx, out_d, n_frames, n_channels, sample_rate, Params::mark_sample_rate, ctx->ws_rate_c.as<float>(), n44)) return r;
      rc = get_watermark_device (ctx, { capi_key (key) }, make_wav (ctx->ws_rate_c.as<float>(), n44, n_channels), rs);
    }
  else
    rc = get_watermark_device (ctx, { capi_key (key) }, make_wav (out_d, n_frames, n_channels), rs);
  ctx->ready.disarm();
  if (rc)
    return rc;
  for (size_t i = 0; i < rs.patterns.size() && i < max_out; i++)
    fill_pattern (rs.patterns[i], out[i]);
  return int (rs.patterns.size());
}

/* WHOLE STREAMS FROM AND TO 16-BIT PCM (include/awm_hip.h awm_add_watermark_s16_d). */
static int g_add_s16_fused_in_use = 0;
extern "C" int awm_debug_add_s16_fused_in_use (void) { return g_add_s16_fused_in_use; }

/* the refusals of both pipeline calls, before anything is enqueued */
static int
check_add_s16 (awm_ctx *ctx, const char *who, const int16_t *pcm_in_d, const int16_t *out_d, size_t n_frames, int n_channels, int sample_rate)
{
  const uintptr_t a = reinterpret_cast<uintptr_t> (pcm_in_d), b = reinterpret_cast<uintptr_t> (out_d);
  const char *bad = nullptr;
  if (n_channels < 1)
    bad = "n_channels < 1";
  else if ((a | b) & 1)
    bad = "an int16 pointer is not 2-byte aligned";
  else if (n_frames && (!pcm_in_d || !out_d))
    bad = "null pointer";
  else if (sample_rate <= 0)
    bad = "bad sample rate";
  else
    {
      const uintptr_t bytes = n_frames * size_t (n_channels) * sizeof (int16_t);
      if (a != b && a < b + bytes && b < a + bytes)
        bad = "the output overlaps the input partially (out_d == pcm_in_d exactly is allowed)";
    }
  if (bad)
    {
      set_error (std::string (who) + ": " + bad);
      return AWM_ERR_ARG;
    }
  if (sample_rate != Params::mark_sample_rate
      && (!rate_converter (ctx, sample_rate, Params::mark_sample_rate).ok() || !rate_converter (ctx, Params::mark_sample_rate, sample_rate).ok()))
    return AWM_ERR_ARG;                                         // (rate_converter has set the message)
  return 0;
}

/* add_full_rate from and to 16-bit PCM: stereo, 4-byte aligned pointers, fixed-ratio tables both ways.  Kernels that exist, composed: the
 * down-resampler reads the int16 values, K2 writes the watermark signal alone, the up-resampler brings it to the rate; the block maxima
 * come from decode (in) + wm with nothing stored, and the last pass computes that sum again, applies the ramp, encodes and stores.  A frame
 * of the input is read for the last time by the thread that stores the same frame of the output: out_d may be pcm_in_d. */
static int
add_full_rate_s16 (awm_ctx *ctx, const int16_t *pcm_in_d, int16_t *out_d, size_t n_frames, const int8_t *frame_mod_dev, double water_delta,
                   int use_limiter, int rate, const RateConverter& down, const RateConverter& up)
{
  const int C = 2;
  const size_t last44 = up.window_start (n_frames - 1) + size_t (up.hl()) + 1;     // (add_full_rate's geometry)
  const size_t F = last44 / Params::frame_size + 1;
  const size_t n44 = (F + 1) * Params::frame_size;
  if (int rc = ctx->ws_rate_a.reserve (n44 * C * sizeof (float))) return rc;
  if (int rc = ctx->ws_rate_b.reserve (n44 * C * sizeof (float))) return rc;
  if (int rc = ctx->ws_rate_c.reserve (n_frames * C * sizeof (float))) return rc;
  float *x44 = ctx->ws_rate_a.as<float>(), *wm44 = ctx->ws_rate_b.as<float>(), *wm = ctx->ws_rate_c.as<float>();
  {
    awmk::ResampleArgs ra = resample_table_args (*down.fixed, C);
    ra.in = reinterpret_cast<const float *> (pcm_in_d);
    ra.n_in = (long long) n_frames;
    ra.out = x44;
    ra.n_out = (long long) n44;
    ProfScope ps (ctx, PROF_RESAMPLE_S16, double (n_frames) * C * 2.0 + double (n44) * C * 4.0);
    AWM_HIP_CHECK (awmk::launch_resample_s16 (ctx->stream, ra));
  }
  {
    awmk::AddMixArgs a {};
    a.pcm_in = x44;
    a.out = wm44;
    a.n_frames = (long long) n44;
    a.n_channels = C;
    a.frame_mod = frame_mod_dev;
    fill_add_mix_common (a, water_delta);
    a.frames_per_span = frames_per_span (ctx, (long long) (F + 1));
    a.delta_only = 1;
    ProfScope ps (ctx, PROF_ADD_MIX, double (n44) * C * 8.0);
    AWM_HIP_CHECK (awmk::launch_add_mix (ctx->stream, ctx->tabs, a));
  }
  if (int rc = resample_device (ctx, up, wm44, F * Params::frame_size, C, wm, n_frames)) return rc;
  const int lim_block = int (size_t (rate) * size_t (Params::limiter_block_size_ms) / 1000);
  const size_t n_blocks = n_frames / lim_block + 2;
  float *block_max = nullptr;
  if (use_limiter)
    {
      if (int rc = ctx->ws_block_max.reserve (n_blocks * sizeof (float))) return rc;
      block_max = ctx->ws_block_max.as<float>();
      if (int rc = awm_add_init_block_max_d (ctx, block_max, n_blocks)) return rc;
      const awmk::MixSegment seg { reinterpret_cast<const float *> (pcm_in_d), wm, nullptr, (long long) n_frames, 0, 0,
                                   reinterpret_cast<unsigned int *> (block_max), 0, (long long) n_blocks };
      AWM_HIP_CHECK (awmk::launch_max_segment_s16 (ctx->stream, seg, C, lim_block));
    }
  return limit_encode_pass (ctx, ctx, wm, out_d, n_frames, C, 0, block_max, 0, n_blocks, lim_block, pcm_in_d);
}

/* the definition, on the context's stream: decode into a float workspace, the float call into a second one, encode into out_d */
static int
add_s16_by_definition (awm_ctx *ctx, const int16_t *pcm_in_d, int16_t *out_d, size_t n_frames, int n_channels, const int8_t *frame_mod_dev,
                       int sample_rate, ReadyMarks *marks = nullptr)
{
  const size_t n_values = n_frames * size_t (n_channels);
  if (int rc = ctx->ws_pcm.reserve (n_values * sizeof (float))) return rc;
  if (int rc = ctx->ws_add_mix.reserve (n_values * sizeof (float))) return rc;
  float *f = ctx->ws_pcm.as<float>(), *g = ctx->ws_add_mix.as<float>();
  {
    ProfScope ps (ctx, PROF_PCM_DECODE, double (n_values) * 6.0);
    AWM_HIP_CHECK (awmk::launch_pcm_decode (ctx->stream, reinterpret_cast<const unsigned char *> (pcm_in_d), f, (long long) n_values,
                                            awmk::PcmFormatDev { 2, 0, 0, 0 }));
  }
  const int rc = sample_rate != Params::mark_sample_rate
               ? add_full_rate (ctx, f, g, n_frames, n_channels, frame_mod_dev, params().water_delta, !params().test_no_limiter, sample_rate)
               : add_full (ctx, f, g, n_frames, n_channels, frame_mod_dev, params().water_delta, !params().test_no_limiter);
  if (rc)
    return rc;
  ProfScope ps (ctx, PROF_PCM_ENCODE, double (n_values) * 6.0);
  AWM_HIP_CHECK (awmk::launch_pcm_encode (ctx->stream, g, reinterpret_cast<unsigned char *> (out_d), (long long) n_values,
                                          awmk::PcmFormatDev { 2, 0, 0, 1 }));
  return 0;
}

/* both pipeline calls behind their checks; marks: awm_add_get_watermark_s16_d at 44.1 kHz (armed by the fused path only) */
static int
add_watermark_s16 (awm_ctx *ctx, FrameModTable *fm, const int16_t *pcm_in_d, int16_t *out_d, size_t n_frames, int n_channels, int sample_rate,
                   ReadyMarks *marks)
{
  g_add_s16_fused_in_use = 0;
  if (!n_frames)
    return 0;
  const int8_t *table = fm->dev.as<int8_t>();
  const int use_limiter = !params().test_no_limiter;
  if (sample_rate == Params::mark_sample_rate)
    {
      g_add_s16_fused_in_use = 1;
      return add_full_s16 (ctx, pcm_in_d, out_d, n_frames, n_channels, table, params().water_delta, use_limiter, nullptr, marks);
    }
  const RateConverter down = rate_converter (ctx, sample_rate, Params::mark_sample_rate);
  const RateConverter up = rate_converter (ctx, Params::mark_sample_rate, sample_rate);
  const int lim_block = int (size_t (sample_rate) * size_t (Params::limiter_block_size_ms) / 1000);
  const bool aligned = ((reinterpret_cast<uintptr_t> (pcm_in_d) | reinterpret_cast<uintptr_t> (out_d)) & 3) == 0;
  if (down.fixed && up.fixed && n_channels == 2 && aligned && lim_block >= 8192 && !ctx->snr_on)
    {
      g_add_s16_fused_in_use = 1;
      return add_full_rate_s16 (ctx, pcm_in_d, out_d, n_frames, table, params().water_delta, use_limiter, sample_rate, down, up);
    }
  return add_s16_by_definition (ctx, pcm_in_d, out_d, n_frames, n_channels, table, sample_rate);
}

int
awm_add_watermark_s16_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const int16_t *pcm_in_d, int16_t *out_d,
                         size_t n_frames, int n_channels, int sample_rate)
{
  AWM_ENTER (ctx);
  if (int rc = check_add_s16 (ctx, "awm_add_watermark_s16_d", pcm_in_d, out_d, n_frames, n_channels, sample_rate))
    return rc;
  FrameModTable *fm = ctx->get_frame_mod (capi_key (key), payload_hex ? payload_hex : "");
  if (!fm)
    return AWM_ERR_ARG;
  return add_watermark_s16 (ctx, fm, pcm_in_d, out_d, n_frames, n_channels, sample_rate, nullptr);
}

int
awm_add_get_watermark_s16_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const int16_t *pcm_in_d, int16_t *out_d,
                             size_t n_frames, int n_channels, int sample_rate, size_t max_out, awm_pattern *out)
{
  AWM_ENTER (ctx);
  if (max_out && !out)
    {
      set_error ("awm_add_get_watermark_s16_d: bad argument");
      return AWM_ERR_ARG;
    }
  if (int rc = check_add_s16 (ctx, "awm_add_get_watermark_s16_d", pcm_in_d, out_d, n_frames, n_channels, sample_rate))
    return rc;
  if (int rc = check_stream_s16 ("awm_add_get_watermark_s16_d", out_d, n_frames, n_channels))       // (what the `get` half would refuse)
    return rc;
  FrameModTable *fm = ctx->get_frame_mod (capi_key (key), payload_hex ? payload_hex : "");
  if (!fm)
    return AWM_ERR_ARG;
  // the hand-over of awm_add_get_watermark_d: `get` starts a chunk once the last pass has passed the chunk's end
  const bool hand_over = sample_rate == Params::mark_sample_rate && n_frames > 0;
  int rc = add_watermark_s16 (ctx, fm, pcm_in_d, out_d, n_frames, n_channels, sample_rate, hand_over ? &ctx->ready : nullptr);
  if (!rc)
    rc = awm_get_watermark_rate_s16_d (ctx, key, out_d, n_frames, n_channels, sample_rate, max_out, out);
  ctx->ready.disarm();
  return rc;
}

/* add_watermark for many independent inputs with one key and payload (BASELINE config 5: a batch of short clips).  A 30 s clip
 * is five launches of a few microseconds of work each: alone on a stream they run one after the other with the GPU mostly idle
 * (65 us per clip), so the clips are dealt to eight lanes.  Ordered after the work queued on the context's stream; the context's
 * stream is ordered after the batch. */
extern "C++" {
namespace {
std::vector<Key>
key_list_from (const uint8_t *keys, int n_keys)
{
  std::vector<Key> list;
  for (int k = 0; k < n_keys; k++)
    list.push_back (capi_key (keys + size_t (k) * Key::SIZE));
  return list;
}
// patterns of a multi-key `get` -> the C arrays; key_of_pattern[j] = position of pattern j's key in the list
int
fill_patterns_keys (const ResultSet& rs, const std::vector<Key>& list, size_t max_out, awm_pattern *out, int *key_of_pattern)
{
  for (size_t i = 0; i < rs.patterns.size() && i < max_out; i++)
    {
      fill_pattern (rs.patterns[i], out[i]);
      if (key_of_pattern)
        {
          key_of_pattern[i] = -1;
          for (size_t k = 0; k < list.size(); k++)
            if (rs.patterns[i].key == list[k])
              {
                key_of_pattern[i] = int (k);
                break;
              }
        }
    }
  return int (rs.patterns.size());
}
}
} // extern "C++"

/* Batches of clips, ONE launch per stage for many clips (fill of the block maxima, K2, K3a, K3b) instead of four launches per clip.
 * A 30 s clip is 1292 frames: alone it is 323 spans of four frames (+ two halo frames each: 1.5 x the transforms) and four launches of
 * 6 - 46 us -- 1024 clips on eight lanes were 26 ms of launches for ~8 ms of memory traffic.  Here the spans are sized for the whole batch
 * (frames_per_span of the batch's frames: ~20 frames per span, 1.1 x the transforms), blockIdx.y is the clip, its arguments come from an
 * array on the device.  Output bit-identical to the per-clip launches (a span's result does not depend on the span length).
 * (measurement knob) awm_debug_set_add_batched (0): the per-clip launches on eight lanes; (1) / (2, default): see add_batch_keys_tables_first */
static int g_add_batched = 2;              // 2: with a key per clip, the tables of all keys first (add_batch_keys_tables_first) | 1: a group's tables while the previous group is watermarked
extern "C" void awm_debug_set_add_batched (int on) { g_add_batched = on; }

static bool
add_clips_batchable (awm_ctx *ctx, size_t n_clips, const float *const *pcm_in_d, float *const *out_d, int n_channels)
{
  if (!g_add_batched || n_channels != 2 || ctx->snr_on || n_clips < 2)
    return false;
  for (size_t i = 0; i < n_clips; i++)
    if ((reinterpret_cast<uintptr_t> (pcm_in_d[i]) & 15) || (reinterpret_cast<uintptr_t> (out_d[i]) & 15))
      return false;
  return true;
}

/* lanes 0 .. n - 1 of the context, each with an ev_sync */
static int
lanes_with_sync (awm_ctx *ctx, int n, std::vector<WorkLane *>& lanes)
{
  lanes.clear();
  for (int i = 0; i < n; i++)
    {
      WorkLane *l = ctx->lane (i);
      if (!l)
        {
          set_error ("cannot create a work lane (stream)");
          return AWM_ERR_HIP;
        }
      if (!l->ev_sync)
        AWM_HIP_CHECK (hipEventCreateWithFlags (&l->ev_sync, hipEventDisableTiming));
      lanes.push_back (l);
    }
  return 0;
}

/* the events of one call (no timing), destroyed with it */
namespace {
struct Events
{
  std::vector<hipEvent_t> ev;
  Events() = default;
  Events (const Events&) = delete;
  Events& operator= (const Events&) = delete;
  ~Events() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy (e); }
  int
  create (size_t n)
  {
    ev = std::vector<hipEvent_t> (n, nullptr);
    for (hipEvent_t& e : ev)
      AWM_HIP_CHECK (hipEventCreateWithFlags (&e, hipEventDisableTiming));
    return 0;
  }
  hipEvent_t operator[] (size_t i) const { return ev[i]; }
};
}

/* Batched arguments of a whole call: staged once (page-locked), copied once; groups then launch on slices of the device arrays. */
struct AddBatchArgs
{
  awmk::AddMixArgs  *d_mix = nullptr;
  awmk::LimiterClip *d_lim = nullptr;
  float             *block_max = nullptr;
  size_t             nb_max = 0;
  std::vector<long long> spans, frames;
  int                L = 4;
};

/* tables: the device table of every clip, or ONE for all (known now; the kernels read them when a group runs) */
static int
add_batch_stage (awm_ctx *ctx, hipStream_t st, size_t n_clips, const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames,
                 const std::vector<const int8_t *>& tables, int use_limiter, AddBatchArgs& b)
{
  const int C = 2;
  long long total_frames1024 = 0;
  size_t max_frames = 0;
  for (size_t i = 0; i < n_clips; i++)
    {
      total_frames1024 += (long long) (n_frames[i] + 1023) / 1024;
      max_frames = std::max (max_frames, n_frames[i]);
    }
  b.L = frames_per_span (ctx, total_frames1024);
  b.nb_max = max_frames / LIMITER_BLOCK + 2;
  const size_t tab_max = awmk::limiter_tab_entries ((long long) max_frames, 0, LIMITER_BLOCK) + 1;
  const size_t arg_bytes = n_clips * (sizeof (awmk::AddMixArgs) + sizeof (awmk::LimiterClip));
  if (int rc = ctx->ws_add_batch.reserve (arg_bytes)) return rc;
  if (int rc = ctx->ws_block_max.reserve (n_clips * b.nb_max * sizeof (float))) return rc;
  if (int rc = ctx->ws_limit_tab.reserve (n_clips * tab_max * sizeof (float2))) return rc;
  if (ctx->ev_add_batch)
    AWM_HIP_CHECK (hipEventSynchronize (ctx->ev_add_batch));            // (an earlier batch's staging has been copied)
  else
    AWM_HIP_CHECK (hipEventCreateWithFlags (&ctx->ev_add_batch, hipEventDisableTiming));
  if (int rc = ctx->pin_add_batch.reserve (arg_bytes)) return rc;
  auto *h_mix = ctx->pin_add_batch.as<awmk::AddMixArgs>();
  auto *h_lim = reinterpret_cast<awmk::LimiterClip *> (h_mix + n_clips);
  b.d_mix = ctx->ws_add_batch.as<awmk::AddMixArgs>();
  b.d_lim = reinterpret_cast<awmk::LimiterClip *> (b.d_mix + n_clips);
  b.block_max = ctx->ws_block_max.as<float>();
  float2 *tabs = ctx->ws_limit_tab.as<float2>();
  b.spans.assign (n_clips, 0);
  b.frames.assign (n_clips, 0);
  for (size_t i = 0; i < n_clips; i++)
    {
      awmk::AddMixArgs a {};
      a.pcm_in = pcm_in_d[i];
      a.out = out_d[i];
      a.n_frames = (long long) n_frames[i];
      a.n_channels = C;
      a.frame_mod = tables.size() == 1 ? tables[0] : tables[i];
      fill_add_mix_common (a, params().water_delta);
      a.block_max = use_limiter ? reinterpret_cast<unsigned int *> (b.block_max + i * b.nb_max) : nullptr;
      a.n_blocks = (long long) (n_frames[i] / LIMITER_BLOCK + 2);
      a.frames_per_span = b.L;
      h_mix[i] = a;
      h_lim[i] = { out_d[i], (long long) n_frames[i], b.block_max + i * b.nb_max, a.n_blocks, tabs + i * tab_max,
                   (long long) awmk::limiter_tab_entries ((long long) n_frames[i], 0, LIMITER_BLOCK) };
      const long long F = (long long) (n_frames[i] + 1023) / 1024;
      b.spans[i] = (F + b.L - 1) / b.L;
      b.frames[i] = (long long) n_frames[i];
    }
  AWM_HIP_CHECK (hipMemcpyAsync (b.d_mix, h_mix, arg_bytes, hipMemcpyHostToDevice, st));
  AWM_HIP_CHECK (hipEventRecord (ctx->ev_add_batch, st));
  return 0;
}

/* clips [i0, i0 + n) of a staged batch on stream st */
static int
add_batch_run (awm_ctx *ctx, hipStream_t st, const AddBatchArgs& b, size_t i0, size_t n, int use_limiter)
{
  if (!n)
    return 0;
  long long max_spans = 0, max_frames = 0;
  double values = 0;
  for (size_t i = i0; i < i0 + n; i++)
    {
      max_spans = std::max (max_spans, b.spans[i]);
      max_frames = std::max (max_frames, b.frames[i]);
      values += double (b.frames[i]) * 2;
    }
  if (use_limiter)
    {
      unsigned int bits;
      std::memcpy (&bits, &LIMITER_CEILING, sizeof (bits));
      AWM_HIP_CHECK (awmk::launch_fill_u32 (st, reinterpret_cast<unsigned int *> (b.block_max + i0 * b.nb_max), bits, n * b.nb_max));
    }
  {
    ProfScope ps (ctx, PROF_ADD_MIX, values * 8.0, st);                            // read + write every sample once
    AWM_HIP_CHECK (awmk::launch_add_mix_batch (st, ctx->tabs, b.d_mix + i0, int (n), max_spans, int (mark_block_frame_count()), int (Params::frames_pad_start)));
  }
  if (use_limiter)
    {
      ProfScope ps (ctx, PROF_LIMITER, values * 8.0, st);
      AWM_HIP_CHECK (awmk::launch_limiter_batch (st, b.d_lim + i0, int (n), max_frames, 2, LIMITER_BLOCK, LIMITER_CEILING));
    }
  return 0;
}

int
awm_add_watermark_batch_d (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, size_t n_clips, const float *const *pcm_in_d,
                           float *const *out_d, const size_t *n_frames, int n_channels)
{
  AWM_ENTER (ctx);
  if (n_clips && (!pcm_in_d || !out_d || !n_frames || n_channels < 1))
    {
      set_error ("awm_add_watermark_batch_d: bad argument");
      return AWM_ERR_ARG;
    }
  FrameModTable *fm = ctx->get_frame_mod (capi_key (key), payload_hex ? payload_hex : "");
  if (!fm)
    return AWM_ERR_ARG;
  if (add_clips_batchable (ctx, n_clips, pcm_in_d, out_d, n_channels))
    {
      const int use_limiter = !params().test_no_limiter;
      AddBatchArgs batch;
      if (int rc = add_batch_stage (ctx, ctx->stream, n_clips, pcm_in_d, out_d, n_frames, { fm->dev.as<int8_t>() }, use_limiter, batch))
        return rc;
      constexpr size_t PER_LAUNCH = 4096;                    // (blockIdx.y <= 65535; a launch of 4096 clips fills the device many times over)
      for (size_t i0 = 0; i0 < n_clips; i0 += PER_LAUNCH)
        if (int rc = add_batch_run (ctx, ctx->stream, batch, i0, std::min (PER_LAUNCH, n_clips - i0), use_limiter))
          return rc;
      return 0;
    }
  constexpr int ADD_LANES = 8;
  const int n_lanes = int (std::min<size_t> (ADD_LANES, n_clips));
  std::vector<WorkLane *> lanes;
  if (int rc = lanes_with_sync (ctx, n_lanes, lanes)) return rc;
  if (n_lanes > 1)
    {
      AWM_HIP_CHECK (hipEventRecord (ctx->ev_sync, ctx->stream));
      for (int i = 1; i < n_lanes; i++)
        AWM_HIP_CHECK (hipStreamWaitEvent (lanes[i]->stream, ctx->ev_sync, 0));
    }
  int rc = 0;
  for (size_t i = 0; i < n_clips && !rc; i++)
    rc = add_full (ctx, pcm_in_d[i], out_d[i], n_frames[i], n_channels, fm->dev.as<int8_t>(), params().water_delta, !params().test_no_limiter,
                   lanes[i % n_lanes]);
  for (int i = 1; i < n_lanes; i++)
    {
      AWM_HIP_CHECK (hipEventRecord (lanes[i]->ev_sync, lanes[i]->stream));
      AWM_HIP_CHECK (hipStreamWaitEvent (ctx->stream, lanes[i]->ev_sync, 0));
    }
  return rc;
}

/* ---- a batch of stream SEGMENTS, each with its own offset and payload (include/awm_hip.h; reference hls.cc:244-279: a few seconds of
 * audio with context on either side, watermarked on request for one subscriber by add_stream_watermark (key, in, out, bits, zero_frames)).
 * The machine is the batched clip path above -- one launch per stage, blockIdx.y = segment --, with three things per segment: the table
 * of its payload (K16p expands the key's template for all distinct payloads of a group in one launch: no table is built on the host), its
 * place in the frame / watermark block grid (first_frame) and in the limiter's (first_sample, first_block).  A segment that begins
 * r = zero_frames % 1024 samples into a frame is staged: "r zeros, then the segment" in an aligned slice of a workspace (one gather
 * launch per batch), K2 and the limiter work there, one scatter launch brings the result home without the r samples.  The scatter is a
 * launch of its own and not the limiter's apply pass writing to the caller's buffer: that pass moves float4 and the caller's buffer is
 * 8 r bytes off the staged slice's 16-byte grid. ---- */
static int g_add_segments_fused_in_use = 0;
extern "C" int awm_debug_add_segments_fused_in_use (void) { return g_add_segments_fused_in_use; }

/* one segment through the tile stream (what every segment of a call that cannot take the fused path goes through) */
static int
add_segment_stream (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, size_t zero_frames, const float *pcm_in_d, float *out_d,
                    size_t n_frames, int C)
{
  constexpr size_t TILE1024 = 128;
  awm_add_stream *s = nullptr;
  if (int rc = add_stream_create (ctx, key, &payload_hex, 1, C, TILE1024, zero_frames, &s))
    return rc;
  struct Guard { awm_add_stream *s; ~Guard() { awm_add_stream_destroy (s); } } guard { s };      // (waits for the stream: the copies below are through)
  const size_t tile = TILE1024 * Params::frame_size;
  size_t pos = 0, written = 0;
  for (;;)
    {
      const size_t got = std::min (tile, n_frames - pos);
      const bool last = pos + got >= n_frames;
      if (got)
        AWM_HIP_CHECK (hipMemcpyAsync (awm_add_stream_input (s), pcm_in_d + pos * C, got * C * sizeof (float), hipMemcpyDeviceToDevice, ctx->stream));
      const float *done[3];
      size_t done_frames[3];
      const int k = add_stream_push (s, got, last, done, done_frames, "awm_add_watermark_segments_d");
      if (k < 0)
        return k;
      for (int i = 0; i < k; i++)
        {
          AWM_HIP_CHECK (hipMemcpyAsync (out_d + written * C, done[i], done_frames[i] * C * sizeof (float), hipMemcpyDeviceToDevice, ctx->stream));
          written += done_frames[i];
        }
      pos += got;
      if (last)
        break;
    }
  return 0;
}

/* ---- segments with a KEY EACH (awm_add_watermark_segments_keys_d, below): what the fused path needs beyond one key.  The tables are
 * the distinct (key, payload) pairs, ordered by key; K16t (hip/keytab.hip) builds the templates of the keys a table group needs, at
 * most KEY_TMPL_LAUNCH per launch, into slot key mod KEY_TMPL_SLOTS of a workspace, and K16p reads table t's template through tmpl_of[t].
 * A group's keys are neighbours and no more than its tables, so within a group no two of them share a slot; a key whose template an
 * earlier group built (the group boundary fell inside its run) is still there.  Geometries K16t does not cover, and
 * awm_debug_set_key_tables_on_device (0), take the host's templates from the context's cache instead: one copy per key. ---- */
constexpr size_t KEY_TMPL_SLOTS = 1024, KEY_TMPL_LAUNCH = 256;

static bool
key_templates_on_device_possible()
{
  return params().mix && params().frames_per_bit == 2 && mark_block_frame_count() == 2226 && mark_sync_frame_count() == 510
         && code_size (ConvBlockType::a, params().payload_size) == KEYTAB_CODE_BITS;
}

struct SegmentKeys
{
  std::vector<std::array<uint8_t, 16>> keys;   // the distinct keys, ascending
  std::vector<int> key_of_table;               // table -> key: non-decreasing
  // set by the fused path
  bool       on_device = false;
  size_t     stride = 0;                       // entries of a template slot (awmk::payload_table_stride)
  size_t     built = 0;                        // keys 0 .. built - 1 have had their templates made
  const int *d_tmpl_of = nullptr;
  const unsigned char *d_aux = nullptr;        // the keys' block without a payload's code (keytab_stage.hh)
  KeytabAux  aux {};

  /* bytes behind the (16-byte aligned) end of the other arguments: tmpl_of, then what K16t reads */
  size_t arg_bytes() const { return key_of_table.size() * sizeof (int) + (on_device ? keytab_aux_layout (keys.size(), false).bytes : 0); }
  int
  reserve (awm_ctx *ctx, size_t table_stride, bool device = g_key_tables_on_device && key_templates_on_device_possible())
  {
    on_device = device;
    stride = table_stride;
    if (int rc = ctx->ws_key_tmpl.reserve (std::min (keys.size(), KEY_TMPL_SLOTS) * stride * sizeof (int16_t))) return rc;
    if (on_device)
      if (int rc = ctx->ws_keytab_scratch.reserve (KEY_TMPL_LAUNCH * awmk::key_table_scratch_bytes())) return rc;
    return 0;
  }
  void
  fill (char *h, const char *d)
  {
    int *tmpl_of = reinterpret_cast<int *> (h);
    for (size_t t = 0; t < key_of_table.size(); t++)
      tmpl_of[t] = int (size_t (key_of_table[t]) % KEY_TMPL_SLOTS);
    d_tmpl_of = reinterpret_cast<const int *> (d);
    if (!on_device)
      return;
    aux = keytab_aux_pack (reinterpret_cast<unsigned char *> (h) + key_of_table.size() * sizeof (int), keys.size(),
                           [this] (size_t k) { return keys[k].data(); });
    d_aux = reinterpret_cast<const unsigned char *> (d) + key_of_table.size() * sizeof (int);
  }
  /* the templates of the keys up to k1 - 1 that are not there yet (the groups come in order: k1 = 1 + the key of a group's last table) */
  int
  build (awm_ctx *ctx, hipStream_t st, size_t k1)
  {
    short *slots = ctx->ws_key_tmpl.as<short>();
    while (built < k1)
      {
        const size_t slot = built % KEY_TMPL_SLOTS;
        if (!on_device)
          {
            FrameModTemplate *tmpl = ctx->get_frame_mod_template (capi_key (keys[built].data()));
            if (!tmpl)
              return AWM_ERR_HIP;
            AWM_HIP_CHECK (hipMemcpyAsync (slots + slot * stride, tmpl->dev.ptr, stride * sizeof (int16_t), hipMemcpyDeviceToDevice, st));
            built++;
            continue;
          }
        const size_t kn = std::min ({ KEY_TMPL_LAUNCH, k1 - built, KEY_TMPL_SLOTS - slot });
        const awmk::KeyTableArgs ka = keytab_args (d_aux, aux, built, kn, ctx->ws_keytab_scratch.as<unsigned char>(), KEY_TMPL_LAUNCH);
        const awmk::KeyTemplateOut out { slots + slot * stride, (long long) stride };
        ProfScope ps (ctx, PROF_KEY_TEMPLATE, double (kn) * stride * sizeof (int16_t), st);       // the templates out, once (721 KB per key)
        AWM_HIP_CHECK (awmk::launch_key_templates (st, ka, out));
        built += kn;
      }
    return 0;
  }
};

/* the conv code of one payload (its parsed bits) behind `coded`: 2 x n_code bytes 0 / 1, the A block's then the B block's */
static int
payload_code_append (const std::vector<int>& bits, size_t n_code, std::vector<unsigned char>& coded)
{
  for (ConvBlockType type : { ConvBlockType::a, ConvBlockType::b })
    {
      const std::vector<int> code = code_encode (type, bits);
      if (code.size() != n_code)
        {
          set_error ("conv code of unexpected size");
          return AWM_ERR_GENERIC;
        }
      for (int c : code)
        coded.push_back ((unsigned char) (c & 1));
    }
  return 0;
}

/* what both segment entry points check before anything is enqueued (fn: the entry point, for the messages), and the distinct payloads'
 * codes: payload_index[i] = index of segment i's payload among the distinct ones, coded = [distinct][2 (A, B)][n_code] bytes.  T: the sample
 * type, float or int16_t -- the buffers of a segment are n C sizeof (T) bytes, and an int16 buffer at an odd address is refused */
extern "C++" {
template<class T> static int
segments_check (awm_ctx *ctx, const char *fn, const uint8_t key[16], size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                const T *const *pcm_in_d, T *const *out_d, const size_t *n_frames, int n_channels, std::vector<size_t>& payload_index,
                std::vector<unsigned char>& coded, size_t& n_code)
{
  if (!key || !payload_hex || !zero_frames || !pcm_in_d || !out_d || !n_frames || n_channels < 1)
    {
      set_error (string_printf ("%s: bad argument", fn));
      return AWM_ERR_ARG;
    }
  if (ctx->snr_on)
    {
      set_error (string_printf ("%s: not available while the SNR meter is armed (awm_ctx_snr_begin)", fn));
      return AWM_ERR_ARG;
    }
  // everything is checked before anything is enqueued
  const size_t C = size_t (n_channels);
  for (size_t i = 0; i < n_segments; i++)
    if (!payload_hex[i] || (n_frames[i] && (!pcm_in_d[i] || !out_d[i])))
      {
        set_error (string_printf ("%s: null pointer at index %zu", fn, i));
        return AWM_ERR_ARG;
      }
  if (std::is_same<T, int16_t>::value)
    for (size_t i = 0; i < n_segments; i++)
      if (n_frames[i] && ((reinterpret_cast<uintptr_t> (pcm_in_d[i]) | reinterpret_cast<uintptr_t> (out_d[i])) & 1))
        {
          set_error (string_printf ("%s: a buffer of 16-bit samples at an odd address at index %zu", fn, i));
          return AWM_ERR_ARG;
        }
  // the distinct payloads in order of appearance: parse_payload + code_encode (A and B) is all the host does per payload
  n_code = code_size (ConvBlockType::a, params().payload_size);
  std::map<std::string, size_t> distinct;
  payload_index.assign (n_segments, 0);
  coded.clear();
  for (size_t i = 0; i < n_segments; i++)
    {
      auto it = distinct.find (payload_hex[i]);
      if (it == distinct.end())
        {
          const std::vector<int> bits = parse_payload (payload_hex[i]);
          if (bits.empty())
            {
              set_error (string_printf ("%s: cannot parse payload '%s' at index %zu", fn, payload_hex[i], i));
              return AWM_ERR_ARG;
            }
          if (!n_frames[i])                                // (a segment without samples: its payload is checked, no table is made for it)
            continue;
          if (int rc = payload_code_append (bits, n_code, coded)) return rc;
          it = distinct.emplace (payload_hex[i], distinct.size()).first;
        }
      payload_index[i] = it->second;
    }
  // Inputs may alias each other (the same segment for many subscribers), an output may overlap nothing: one sweep over the buffers by
  // address, with the furthest end of any buffer and of any output seen so far
  {
    struct Range { uintptr_t a, b; size_t seg; bool out; };
    std::vector<Range> ranges;
    for (size_t i = 0; i < n_segments; i++)
      if (n_frames[i])
        {
          const uintptr_t bytes = n_frames[i] * C * sizeof (T);
          ranges.push_back ({ reinterpret_cast<uintptr_t> (pcm_in_d[i]), reinterpret_cast<uintptr_t> (pcm_in_d[i]) + bytes, i, false });
          ranges.push_back ({ reinterpret_cast<uintptr_t> (out_d[i]), reinterpret_cast<uintptr_t> (out_d[i]) + bytes, i, true });
        }
    std::sort (ranges.begin(), ranges.end(), [] (const Range& x, const Range& y) { return x.a < y.a; });
    uintptr_t end_any = 0, end_out = 0;
    size_t seg_any = 0, seg_out = 0;
    for (const Range& r : ranges)
      {
        if (r.out ? r.a < end_any : r.a < end_out)
          {
            set_error (string_printf ("%s: the output of segment %zu overlaps a buffer of segment %zu", fn,
                                      r.out ? r.seg : seg_out, r.out ? seg_any : r.seg));
            return AWM_ERR_ARG;
          }
        if (r.b > end_any) { end_any = r.b; seg_any = r.seg; }
        if (r.out && r.b > end_out) { end_out = r.b; seg_out = r.seg; }
      }
  }
  return 0;
}
} // extern "C++"

/* the segments with samples, by payload: the segments of a group of payloads are neighbours */
static void
segments_by_payload (size_t n_segments, const size_t *n_frames, const std::vector<size_t>& payload_index, std::vector<size_t>& segs,
                     std::vector<size_t>& payload_of)
{
  segs.clear();
  for (size_t i = 0; i < n_segments; i++)
    if (n_frames[i])
      segs.push_back (i);
  std::stable_sort (segs.begin(), segs.end(), [&] (size_t x, size_t y) { return payload_index[x] < payload_index[y]; });
  payload_of.resize (segs.size());
  for (size_t i = 0; i < segs.size(); i++)
    payload_of[i] = payload_index[segs[i]];
}

/* ---- the same at another sample rate: awm_add_watermark_segments_rate_d (include/awm_hip.h).  add_full_rate's stages
 * -- resample down, K2 for the watermark signal alone, resample up, mix + block maxima, limiter -- run on the WINDOW of each segment that
 * awm_add_segment_plan describes: the 44.1 kHz frames around the segment, at their global indices (table row, resampler phase, limiter
 * block and phase).  Nothing in front of the window is stored or computed. ---- */
struct SegmentWindow
{
  awm_segment_plan p;
  size_t Z, n, pre;            // zero_frames, n_frames, samples of watermark alone in front (Z - mix_first)
  size_t slice_frames;         // 44.1 kHz frames K2 runs over
  size_t n_tab;                // limiter ramp table entries
};

static int
segment_window (int rate, size_t zero_frames, size_t n_frames, SegmentWindow& w)
{
  if (int rc = awm_add_segment_plan (rate, zero_frames, n_frames, &w.p))
    return rc;
  w.Z = zero_frames;
  w.n = n_frames;
  w.pre = zero_frames - size_t (w.p.mix_first);
  w.slice_frames = size_t (w.p.slice_last - w.p.slice_first + 1);
  w.n_tab = awmk::limiter_tab_entries ((long long) n_frames, (long long) zero_frames, int (w.p.limiter_block));
  return 0;
}

static awmk::ResampleArgs
resample_table_args (const ResampleTable& t, int C)
{
  awmk::ResampleArgs ra {};
  ra.n_channels = C;
  ra.ctab = t.ctab.as<float>();
  ra.hl = t.hl;
  ra.np = t.np;
  ra.step = t.step;
  return ra;
}

// the three slices of a window: `in` = the segment, x44 / wm44 = slice_frames * 1024 frames each, wm = pre + n frames
// (T = int16_t: `in` of the slice holds the address of the int16 values, launch_resample_slices_s16)
extern "C++" {
template<class T> static awmk::ResampleSlice
window_down_slice (const SegmentWindow& w, const T *in, int C, float *x44)
{
  return { reinterpret_cast<const float *> (in + size_t (w.p.in_first) * C), (long long) (w.p.in_last - w.p.in_first + 1), (long long) (w.Z + w.p.in_first),
           (long long) w.p.down_first, (long long) (w.slice_frames * Params::frame_size), x44 };
}
} // extern "C++"
static awmk::AddMixArgs
window_mix_args (const SegmentWindow& w, const float *x44, float *wm44, int C, const int8_t *frame_mod, double water_delta, int frames_per_span)
{
  awmk::AddMixArgs a {};
  a.pcm_in = x44;
  a.out = wm44;
  a.n_frames = (long long) (w.slice_frames * Params::frame_size);
  a.n_channels = C;
  a.frame_mod = frame_mod;
  fill_add_mix_common (a, water_delta);
  a.first_frame = (long long) w.p.slice_first;
  a.frames_per_span = frames_per_span;
  a.delta_only = 1;
  return a;
}
static awmk::ResampleSlice
window_up_slice (const SegmentWindow& w, const float *wm44, int C, float *wm)
{
  // only the complete frames are handed over: a read outside them would come back as zero and show in the result
  return { wm44 + size_t (w.p.frame_first - w.p.slice_first) * Params::frame_size * C,
           (long long) ((w.p.frame_last - w.p.frame_first + 1) * Params::frame_size), (long long) (w.p.frame_first * Params::frame_size),
           (long long) w.p.mix_first, (long long) (w.pre + w.n), wm };
}

/* one segment through the single-stream launchers (what every segment of a call that cannot take the fused path goes through) */
static int
add_segment_rate (awm_ctx *ctx, const ResampleTable& down, const ResampleTable& up, const uint8_t key[16], const char *payload_hex, size_t zero_frames,
                  const float *pcm_in_d, float *out_d, size_t n_frames, int C, int rate)
{
  SegmentWindow w;
  if (int rc = segment_window (rate, zero_frames, n_frames, w))
    return rc;
  FrameModTable *fm = ctx->get_frame_mod (capi_key (key), payload_hex);
  if (!fm)
    return AWM_ERR_ARG;
  const int use_limiter = !params().test_no_limiter, lim_block = int (w.p.limiter_block);
  const size_t n44 = w.slice_frames * Params::frame_size;
  if (int rc = ctx->ws_rate_a.reserve (n44 * C * sizeof (float))) return rc;
  if (int rc = ctx->ws_rate_b.reserve (n44 * C * sizeof (float))) return rc;
  if (int rc = ctx->ws_rate_c.reserve ((w.pre + n_frames) * C * sizeof (float))) return rc;
  float *x44 = ctx->ws_rate_a.as<float>(), *wm44 = ctx->ws_rate_b.as<float>(), *wm = ctx->ws_rate_c.as<float>();
  hipStream_t st = ctx->stream;
  {
    const awmk::ResampleSlice s = window_down_slice (w, pcm_in_d, C, x44);
    ProfScope ps (ctx, PROF_RESAMPLE, double (s.n_in + s.n_out) * C * 4.0);
    AWM_HIP_CHECK (awmk::launch_resample_slice (st, resample_table_args (down, C), s));
  }
  {
    const awmk::AddMixArgs a = window_mix_args (w, x44, wm44, C, fm->dev.as<int8_t>(), params().water_delta, frames_per_span (ctx, (long long) w.slice_frames));
    ProfScope ps (ctx, PROF_ADD_MIX, double (n44) * C * 8.0);
    AWM_HIP_CHECK (awmk::launch_add_mix (st, ctx->tabs, a));
  }
  {
    const awmk::ResampleSlice s = window_up_slice (w, wm44, C, wm);
    ProfScope ps (ctx, PROF_RESAMPLE, double (s.n_in + s.n_out) * C * 4.0);
    AWM_HIP_CHECK (awmk::launch_resample_slice (st, resample_table_args (up, C), s));
  }
  const size_t n_blocks = size_t (w.p.n_blocks);
  if (use_limiter)
    {
      if (int rc = ctx->ws_block_max.reserve (n_blocks * sizeof (float))) return rc;
      if (int rc = awm_add_init_block_max_d (ctx, ctx->ws_block_max.as<float>(), n_blocks)) return rc;
    }
  const awmk::MixSegment ms { pcm_in_d, wm, out_d, (long long) n_frames, (long long) w.pre, (long long) zero_frames,
                              use_limiter ? ctx->ws_block_max.as<unsigned int>() : nullptr, (long long) w.p.first_block, (long long) n_blocks };
  AWM_HIP_CHECK (awmk::launch_mix_max_segment (st, ms, C, lim_block));
  if (use_limiter)
    {
      if (int rc = ctx->ws_limit_tab.reserve ((w.n_tab + 1) * sizeof (float2))) return rc;
      ProfScope ps (ctx, PROF_LIMITER, double (n_frames) * C * 8.0);
      AWM_HIP_CHECK (awmk::launch_limiter (st, out_d, (long long) n_frames, C, (long long) zero_frames, ctx->ws_block_max.as<float>(),
                                           (long long) w.p.first_block, (long long) n_blocks, lim_block, LIMITER_CEILING,
                                           ctx->ws_limit_tab.as<float2>(), w.n_tab));
    }
  return 0;
}

constexpr size_t WS_MAX_FLOATS = size_t (1) << 28;         // 1 GiB per workspace (44.1 kHz slices, watermark frames, watermark signals): a batch that would need more is split

/* a segment whose window alone exceeds a workspace (about 50 minutes of stereo) cannot be part of a batch: such a call goes segment by
 * segment, where the workspaces grow to what the segment needs */
static bool
segments_rate_fit_the_workspaces (size_t n_segments, const size_t *zero_frames, const size_t *n_frames, int C, int rate)
{
  for (size_t i = 0; i < n_segments; i++)
    {
      SegmentWindow w;
      if (n_frames[i] && (segment_window (rate, zero_frames[i], n_frames[i], w) || w.slice_frames * Params::frame_size * C > WS_MAX_FLOATS
                          || (w.pre + w.n) * C + 3 > WS_MAX_FLOATS))
        return false;
    }
  return true;
}

/* ---- segments with a key each: awm_add_watermark_segments_keys_d / _rate_d (include/awm_hip.h).  The fused path
 * below with one thing more per table: the template it is expanded from (SegmentKeys). ---- */
static bool
segments_share_one_key (const uint8_t *keys, size_t n_segments)
{
  for (size_t i = 1; i < n_segments; i++)
    if (std::memcmp (keys, keys + 16 * i, 16))
      return false;
  return true;
}

/* the segments with samples by (key, payload); the tables = the distinct pairs in that order (table_of[i]: the table of ordered segment
 * i, coded_tables: their codes), the distinct keys and the key of every table (mk) */
static void
segments_by_key_and_payload (size_t n_segments, const uint8_t *keys, const size_t *n_frames, const std::vector<size_t>& payload_index,
                             const std::vector<unsigned char>& coded, size_t n_code, SegmentKeys& mk, std::vector<size_t>& segs,
                             std::vector<size_t>& table_of, std::vector<unsigned char>& coded_tables)
{
  segs.clear();
  for (size_t i = 0; i < n_segments; i++)
    if (n_frames[i])
      segs.push_back (i);
  std::stable_sort (segs.begin(), segs.end(), [&] (size_t x, size_t y) {
    const int c = std::memcmp (keys + 16 * x, keys + 16 * y, 16);
    return c ? c < 0 : payload_index[x] < payload_index[y];
  });
  table_of.resize (segs.size());
  coded_tables.clear();
  for (size_t i = 0; i < segs.size(); i++)
    {
      const uint8_t *key = keys + 16 * segs[i];
      const bool new_key = !i || std::memcmp (key, keys + 16 * segs[i - 1], 16);
      if (new_key)
        {
          mk.keys.emplace_back();
          std::memcpy (mk.keys.back().data(), key, 16);
        }
      if (new_key || payload_index[segs[i]] != payload_index[segs[i - 1]])
        {
          mk.key_of_table.push_back (int (mk.keys.size() - 1));
          const unsigned char *code = coded.data() + payload_index[segs[i]] * 2 * n_code;
          coded_tables.insert (coded_tables.end(), code, code + 2 * n_code);
        }
      table_of[i] = mk.key_of_table.size() - 1;
    }
}

/* ---- THE SEGMENT BATCHES, all ten entry points: one key or a key each, float or signed 16-bit PCM, one sample rate for the call or one
 * per segment (include/awm_hip.h; DESIGN.md sections 9.2, 9.3, 9.6, 9.7, 9.8).  One body (add_segments_any) checks, decides between the
 * fused path and segment by segment, and orders the segments by their tables; one fused function (add_segments_fused) plans, uploads and
 * runs the batches of the two KINDS of segment:
 *   at 44.1 kHz     K2 mixes in place; a segment that begins r = zero_frames % 1024 samples into a frame is staged (above)
 *   the window kind at another rate: add_full_rate's stages on the window of each segment (SegmentWindow)
 * A call with a rate per segment has both kinds (no identity resampler for 44.1 kHz: (1e-20f + x) - 1e-20f is not x for every float); its
 * window kind carries the rate-dependent values -- the resamplers' tables and geometry, the limiter block -- in the descriptors
 * (kernels.hh RateResampleSlice ...) and takes the `_rates` launchers, so its batches are not split by rate.  A call at one rate takes the
 * one-rate descriptors and launchers.  Both kinds read the same payload tables: K16p runs once per table group, K16t once per key. ---- */
static bool rates_all_equal (size_t n, const int *sample_rates);      // (with the `get` batches, below)

constexpr size_t SEGMENTS_PER_LAUNCH = 4096;               // (blockIdx.y <= 65535; a launch of 4096 clips fills the device many times over)
constexpr size_t SEGMENT_TABLE_GROUP = 1024;               // distinct payloads whose tables exist at a time (~370 MB at the default geometry)

struct RateTables
{
  const ResampleTable *down = nullptr, *up = nullptr;
  int limiter_block = 0;
};

/* the kernel arguments of a fused call: arrays one behind the other, each on a 16-byte boundary, in the context's page-locked block and
 * in its twin on the device.  take() while the sizes are known and nothing else, reserve() once, host() / dev() of what was taken,
 * upload() once: one copy per call */
extern "C++" {
template<class D> struct SegmentArgArray { size_t off; };
struct SegmentArgs
{
  size_t bytes = 0;
  char  *h = nullptr, *d = nullptr;

  template<class D> SegmentArgArray<D>
  take (size_t n)
  {
    const SegmentArgArray<D> a { bytes };
    bytes = (bytes + n * sizeof (D) + 15) / 16 * 16;
    return a;
  }
  template<class D> D *host (SegmentArgArray<D> a) const { return reinterpret_cast<D *> (h + a.off); }
  template<class D> const D *dev (SegmentArgArray<D> a) const { return reinterpret_cast<const D *> (d + a.off); }
  int
  reserve (awm_ctx *ctx)
  {
    if (int rc = ctx->ws_add_batch.reserve (bytes)) return rc;
    if (ctx->ev_add_batch)
      AWM_HIP_CHECK (hipEventSynchronize (ctx->ev_add_batch));          // (an earlier batch's staging has been copied)
    else
      AWM_HIP_CHECK (hipEventCreateWithFlags (&ctx->ev_add_batch, hipEventDisableTiming));
    if (int rc = ctx->pin_add_batch.reserve (bytes)) return rc;
    h = ctx->pin_add_batch.as<char>();
    d = ctx->ws_add_batch.as<char>();
    return 0;
  }
  int
  upload (awm_ctx *ctx, hipStream_t st)
  {
    AWM_HIP_CHECK (hipMemcpyAsync (d, h, bytes, hipMemcpyHostToDevice, st));
    AWM_HIP_CHECK (hipEventRecord (ctx->ev_add_batch, st));
    return 0;
  }
};
} // extern "C++"

/* the tables of one group into ws_keytab (K16p, no table is built on the host): n_tables of them from `coded` on, expanded from the one
 * key's template or, with a key per segment, from the templates of their keys, which are built first where they are missing (K16t) */
static int
segment_table_group (awm_ctx *ctx, hipStream_t st, const FrameModTemplate *tmpl, SegmentKeys *mk, size_t first_table, size_t n_tables,
                     const unsigned char *coded_dev, size_t n_code)
{
  const size_t block_frames = mark_block_frame_count(), table_stride = awmk::payload_table_stride (block_frames);
  awmk::PayloadTableArgs pa {};
  pa.n_payloads = int (n_tables);
  pa.tmpl = mk ? ctx->ws_key_tmpl.as<short>() : tmpl->dev.as<short>();
  if (mk)
    {
      if (int rc = mk->build (ctx, st, size_t (mk->key_of_table[first_table + n_tables - 1]) + 1)) return rc;
      pa.tmpl_of = mk->d_tmpl_of + first_table;
      pa.tmpl_stride = (long long) table_stride;
    }
  pa.coded = coded_dev + first_table * 2 * n_code;
  pa.tables = ctx->ws_keytab.as<signed char>();
  pa.table_stride = (long long) table_stride;
  pa.half_entries = int (block_frames * Params::n_bands);
  pa.n_code = int (n_code);
  ProfScope ps (ctx, PROF_PAYLOAD_TAB, double (pa.n_payloads) * table_stride, st);          // the tables out, once
  AWM_HIP_CHECK (awmk::launch_payload_tables (st, pa));
  return 0;
}

/* the fused path (stereo): segs = the segments with samples, ordered by payload; payload_of[i] = index of segment i's payload among the
 * distinct ones; coded = their codes, [distinct][2 (A, B)][n_code] bytes.  With a key per segment (mk; key is not used): ordered by (key,
 * payload), and "payload" reads "(key, payload) pair" -- a table each, expanded from the template of its key.
 * MIXED: rates[s] is the rate of segment s (a call with a rate per segment); else rates[0] is the rate of all of them.
 * T = int16_t: segments of signed 16-bit PCM.
 *   at 44.1 kHz     EVERY segment is staged, the r == 0 ones too -- the gather decodes on its way into ws_seg_in, K2 and the limiter's table
 *                   run on the slices as for float --, and the scatter is the limiter's apply pass with a 16-bit sink: it reads the
 *                   un-limited mix from ws_seg_out behind the r samples, scales, encodes and stores to out_d
 *   the window kind the down-resampler reads the int16 segments, K2 and the up-resampler are as for float, the mix is computed twice and
 *                   stored never -- once for the block maxima, once in the last pass, which scales by the limiter's ramp, encodes and
 *                   stores int16 to out_d.  No workspace beyond ws_rate_a / b / c */
extern "C++" {
template<class T, bool MIXED> static int
add_segments_fused (awm_ctx *ctx, const std::map<int, RateTables>& rate_tables, const uint8_t key[16], const std::vector<size_t>& segs,
                    const std::vector<size_t>& payload_of, const std::vector<unsigned char>& coded, size_t n_code, const size_t *zero_frames,
                    const T *const *pcm_in_d, T *const *out_d, const size_t *n_frames, const int *rates, SegmentKeys *mk)
{
  constexpr bool S16 = std::is_same<T, int16_t>::value;
  typedef typename std::conditional<S16, awmk::LimitEncodeSegment, awmk::SegmentCopy>::type Scatter;
  // the window kind's descriptors: those of the one-rate launchers, in a mixed call each with its rate's values behind it
  typedef typename std::conditional<MIXED, awmk::RateResampleSlice, awmk::ResampleSlice>::type WSlice;
  typedef typename std::conditional<MIXED, awmk::RateMixSegment, awmk::MixSegment>::type WMix;
  typedef typename std::conditional<MIXED, awmk::RateLimiterClip, awmk::LimiterClip>::type WLim;
  typedef typename std::conditional<MIXED, awmk::RateLimitEncodeSegment, awmk::LimitEncodeSegment>::type WEnc;
  constexpr size_t PER_LAUNCH = SEGMENTS_PER_LAUNCH, TABLE_GROUP = SEGMENT_TABLE_GROUP;
  constexpr size_t STAGE_MAX_FLOATS = size_t (1) << 28;    // staged samples per batch and direction (1 GiB): a batch that would need more is split
  const int C = 2;
  const size_t FRAME = Params::frame_size, n_distinct = coded.size() / (2 * n_code);
  const int use_limiter = !params().test_no_limiter;
  const size_t block_frames = mark_block_frame_count();
  const size_t table_stride = awmk::payload_table_stride (block_frames);
  hipStream_t st = ctx->stream;

  FrameModTemplate *tmpl = mk ? nullptr : ctx->get_frame_mod_template (capi_key (key));      // (a key per segment: SegmentKeys' templates)
  if (!tmpl && !mk)
    return AWM_ERR_HIP;

  // the two kinds, each in the order of the tables
  auto rate_of = [&] (size_t s) { return rates[MIXED ? s : 0]; };
  std::vector<size_t> at_rate, at_44;
  for (size_t i = 0; i < segs.size(); i++)
    (rate_of (segs[i]) == Params::mark_sample_rate ? at_44 : at_rate).push_back (i);
  const size_t nr = at_rate.size(), nf = at_44.size();
  auto group_of = [&] (size_t i) { return payload_of[i] / TABLE_GROUP; };
  size_t max_total = 0, tab_total = 0;                     // block maxima and ramp table entries: the window kind's first, then 44.1 kHz

  // the window kind: the window of every segment and the batches: consecutive segments (in table order) of one table group, at most
  // PER_LAUNCH of them, none of the three workspaces beyond WS_MAX_FLOATS.  Segments of a batch that agree in input, length, offset and
  // rate share one down-resampled slice
  struct RSeg { SegmentWindow w; const RateTables *t; size_t down, x44_off, wm44_off, wm_off, max_off, tab_off; };
  struct RBatch { size_t i0, i1, d0, d1, x44_floats, wm44_floats, wm_floats, max_n44, max_out, max_tab, max_len; long long frames1024; int min_block; };
  std::vector<RSeg> rgeo (nr);
  std::vector<RBatch> rbatches;
  std::vector<size_t> down_owner;                          // segment (of this kind) whose window a down slice is made for
  std::map<std::tuple<const T *, size_t, size_t, int>, size_t> shared;
  for (size_t k = 0; k < nr; k++)
    {
      RSeg& g = rgeo[k];
      const size_t i = at_rate[k], s = segs[i];
      g.t = MIXED ? &rate_tables.at (rate_of (s)) : &rate_tables.begin()->second;
      if (int rc = segment_window (rate_of (s), zero_frames[s], n_frames[s], g.w))
        return rc;
      // (a segment that alone exceeds a workspace never gets here: segments_rate_fit_the_workspaces)
      const size_t n44_floats = g.w.slice_frames * FRAME * C, wm_floats = ((g.w.pre + g.w.n) * C + 3) / 4 * 4;
      const auto id = std::make_tuple (pcm_in_d[s], n_frames[s], zero_frames[s], rate_of (s));
      bool fresh = rbatches.empty() || k - rbatches.back().i0 >= PER_LAUNCH || group_of (i) != group_of (at_rate[rbatches.back().i0]);
      if (!fresh)
        {
          const RBatch& b = rbatches.back();
          const bool have = shared.count (id) > 0;
          fresh = b.wm44_floats + n44_floats > WS_MAX_FLOATS || b.wm_floats + wm_floats > WS_MAX_FLOATS || (!have && b.x44_floats + n44_floats > WS_MAX_FLOATS);
        }
      if (fresh)
        {
          rbatches.push_back ({ k, k, down_owner.size(), down_owner.size(), 0, 0, 0, 0, 0, 0, 0, 0, g.t->limiter_block });
          shared.clear();
        }
      RBatch& b = rbatches.back();
      auto it = shared.find (id);
      if (it == shared.end())
        {
          it = shared.emplace (id, k).first;
          g.x44_off = b.x44_floats;
          b.x44_floats += n44_floats;
          down_owner.push_back (k);
          b.d1 = down_owner.size();
        }
      else
        g.x44_off = rgeo[it->second].x44_off;
      g.wm44_off = b.wm44_floats;
      b.wm44_floats += n44_floats;
      g.wm_off = b.wm_floats;
      b.wm_floats += wm_floats;
      g.max_off = max_total;
      g.tab_off = tab_total;
      max_total += size_t (g.w.p.n_blocks);
      tab_total += g.w.n_tab + 1;
      b.i1 = k + 1;
      b.max_n44 = std::max (b.max_n44, g.w.slice_frames * FRAME);
      b.max_out = std::max (b.max_out, g.w.pre + g.w.n);
      b.max_tab = std::max (b.max_tab, g.w.n_tab);
      b.max_len = std::max (b.max_len, g.w.n);
      b.frames1024 += (long long) g.w.slice_frames;
      b.min_block = std::min (b.min_block, g.t->limiter_block);
    }
  size_t x44_max = 0, wm44_max = 0, wm_max = 0;
  long long frames_max = 0;
  for (const RBatch& b : rbatches)
    {
      x44_max = std::max (x44_max, b.x44_floats);
      wm44_max = std::max (wm44_max, b.wm44_floats);
      wm_max = std::max (wm_max, b.wm_floats);
      frames_max = std::max (frames_max, b.frames1024);
    }
  const int L_rate = frames_per_span (ctx, frames_max);
  const size_t n_down = down_owner.size();

  // at 44.1 kHz: the geometry of every segment and the batches: consecutive segments (in table order) of one table group, at most
  // PER_LAUNCH of them, no more than STAGE_MAX_FLOATS staged
  struct FSeg { size_t r, skipped, len, first_block, n_blocks, n_tab, max_off, tab_off, stage_off; };
  struct FBatch { size_t i0, i1, g0, g1, stage_floats, max_len, max_tab; };
  std::vector<FSeg> fgeo (nf);
  std::vector<FBatch> fbatches;
  size_t stage_max = 0, n_staged = 0;
  long long total_frames1024 = 0;
  for (size_t k = 0; k < nf; k++)
    {
      const size_t i = at_44[k], zf = zero_frames[segs[i]];
      FSeg& g = fgeo[k];
      g.r = zf % FRAME;
      g.skipped = zf - g.r;
      g.len = g.r + n_frames[segs[i]];                     // the stream behind the whole frames of zeros: r zeros, then the segment
      g.first_block = g.skipped / LIMITER_BLOCK;
      g.n_blocks = (g.skipped + g.len) / LIMITER_BLOCK + 2 - g.first_block;
      g.n_tab = awmk::limiter_tab_entries ((long long) g.len, (long long) g.skipped, LIMITER_BLOCK);
      g.max_off = max_total;
      g.tab_off = tab_total;
      max_total += g.n_blocks;
      tab_total += g.n_tab + 1;
      total_frames1024 += (long long) ((g.len + FRAME - 1) / FRAME);
      const bool stage = g.r || S16;
      const size_t stage_floats = stage ? (g.len * 2 + 3) / 4 * 4 : 0;
      if (fbatches.empty() || k - fbatches.back().i0 >= PER_LAUNCH || group_of (i) != group_of (at_44[fbatches.back().i0])
          || (fbatches.back().stage_floats && fbatches.back().stage_floats + stage_floats > STAGE_MAX_FLOATS))
        fbatches.push_back ({ k, k, n_staged, n_staged, 0, 0, 0 });
      FBatch& b = fbatches.back();
      g.stage_off = b.stage_floats;
      b.stage_floats += stage_floats;
      b.i1 = k + 1;
      b.max_len = std::max (b.max_len, g.len);
      b.max_tab = std::max (b.max_tab, g.n_tab);
      if (stage)
        b.g1 = ++n_staged;
      stage_max = std::max (stage_max, b.stage_floats);
    }
  const int L_44 = frames_per_span (ctx, total_frames1024);

  // one page-locked block, one upload: the kernel arguments of every stage of both kinds, the gather / scatter lists of the staged
  // segments, the payloads' codes and what the keys' templates are built from
  SegmentArgs args;
  const auto a_down = args.take<WSlice> (n_down), a_up = args.take<WSlice> (nr);
  const auto a_rmix = args.take<awmk::AddMixArgs> (nr);
  const auto a_mm = args.take<WMix> (nr);
  const auto a_rlim = args.take<WLim> (nr);
  const auto a_enc = args.take<WEnc> (S16 ? nr : 0);
  const auto a_fmix = args.take<awmk::AddMixArgs> (nf);
  const auto a_flim = args.take<awmk::LimiterClip> (nf);
  const auto a_gather = args.take<awmk::SegmentCopy> (n_staged);
  const auto a_scatter = args.take<Scatter> (n_staged);
  const auto a_coded = args.take<unsigned char> (coded.size());
  if (mk)
    if (int rc = mk->reserve (ctx, table_stride)) return rc;
  const auto a_keys = args.take<char> (mk ? mk->arg_bytes() : 0);
  if (int rc = ctx->ws_keytab.reserve (std::min (n_distinct, TABLE_GROUP) * table_stride)) return rc;
  if (nr)
    {
      if (int rc = ctx->ws_rate_a.reserve (x44_max * sizeof (float))) return rc;
      if (int rc = ctx->ws_rate_b.reserve (wm44_max * sizeof (float))) return rc;
      if (int rc = ctx->ws_rate_c.reserve (wm_max * sizeof (float))) return rc;
    }
  if (use_limiter)
    {
      if (int rc = ctx->ws_block_max.reserve (max_total * sizeof (float))) return rc;
      if (int rc = ctx->ws_limit_tab.reserve (tab_total * sizeof (float2))) return rc;
    }
  if (stage_max)
    {
      if (int rc = ctx->ws_seg_in.reserve (stage_max * sizeof (float))) return rc;
      if (int rc = ctx->ws_seg_out.reserve (stage_max * sizeof (float))) return rc;
    }
  if (int rc = args.reserve (ctx)) return rc;
  WSlice *h_down = args.host (a_down), *h_up = args.host (a_up);
  const WSlice *d_down = args.dev (a_down), *d_up = args.dev (a_up);
  const awmk::AddMixArgs *d_rmix = args.dev (a_rmix), *d_fmix = args.dev (a_fmix);
  const WMix *d_mm = args.dev (a_mm);
  const WLim *d_rlim = args.dev (a_rlim);
  const WEnc *d_enc = args.dev (a_enc);
  const awmk::LimiterClip *d_flim = args.dev (a_flim);
  const awmk::SegmentCopy *d_gather = args.dev (a_gather);
  const Scatter *d_scatter = args.dev (a_scatter);
  std::memcpy (args.host (a_coded), coded.data(), coded.size());
  if (mk)
    mk->fill (args.host (a_keys), args.dev (a_keys));
  float *x44 = ctx->ws_rate_a.as<float>(), *wm44 = ctx->ws_rate_b.as<float>(), *wm = ctx->ws_rate_c.as<float>();
  float *block_max = ctx->ws_block_max.as<float>();
  float2 *tabs = ctx->ws_limit_tab.as<float2>();
  auto table_of = [&] (size_t i) { return ctx->ws_keytab.as<int8_t>() + (payload_of[i] % TABLE_GROUP) * table_stride; };

  // the window kind's arguments.  A mixed call's slice has its resampler's table and the launch geometry at that rate behind it, its
  // other descriptors the limiter block of their rate
  auto rate_slice = [&] (const awmk::ResampleSlice& s, const ResampleTable& t) -> WSlice {
    if constexpr (MIXED)
      {
        awmk::RateResampleSlice r { s, t.ctab.as<float>(), t.hl, t.np, t.step, 0, 0 };
        awmk::resample_slice_geometry (r, C, true);
        return r;
      }
    else
      return s;
  };
  auto slice_of = [] (const WSlice& r) -> const awmk::ResampleSlice& {
    if constexpr (MIXED)
      return r.s;
    else
      return r;
  };
  auto at_block = [] (auto& slot, const auto& descriptor, int lim_block) {
    if constexpr (MIXED)
      slot = { descriptor, lim_block };
    else
      slot = descriptor;
  };
  for (size_t q = 0; q < n_down; q++)
    {
      const RSeg& g = rgeo[down_owner[q]];
      h_down[q] = rate_slice (window_down_slice (g.w, pcm_in_d[segs[at_rate[down_owner[q]]]], C, x44 + g.x44_off), *g.t->down);
    }
  for (size_t k = 0; k < nr; k++)
    {
      const RSeg& g = rgeo[k];
      const size_t i = at_rate[k], s = segs[i];
      const int lim_block = g.t->limiter_block;
      args.host (a_rmix)[k] = window_mix_args (g.w, x44 + g.x44_off, wm44 + g.wm44_off, C, table_of (i), params().water_delta, L_rate);
      h_up[k] = rate_slice (window_up_slice (g.w, wm44 + g.wm44_off, C, wm + g.wm_off), *g.t->up);
      float *mix_out = nullptr;                                   // (16-bit: no mix is stored; `orig` holds the address of the int16 values)
      if constexpr (!S16)
        mix_out = out_d[s];
      const awmk::MixSegment mm { reinterpret_cast<const float *> (pcm_in_d[s]), wm + g.wm_off, mix_out, (long long) g.w.n, (long long) g.w.pre,
                                  (long long) g.w.Z, use_limiter ? reinterpret_cast<unsigned int *> (block_max + g.max_off) : nullptr,
                                  (long long) g.w.p.first_block, (long long) g.w.p.n_blocks };
      const awmk::LimiterClip lim { mix_out, (long long) g.w.n, use_limiter ? block_max + g.max_off : nullptr, (long long) g.w.p.n_blocks,
                                    use_limiter ? tabs + g.tab_off : nullptr, (long long) g.w.n_tab, (long long) g.w.Z, (long long) g.w.p.first_block };
      at_block (args.host (a_mm)[k], mm, lim_block);
      at_block (args.host (a_rlim)[k], lim, lim_block);
      if constexpr (S16)
        {
          const awmk::LimitEncodeSegment enc { pcm_in_d[s], wm + g.wm_off + g.w.pre * C, out_d[s], (long long) g.w.n, (long long) g.w.Z,
                                               use_limiter ? tabs + g.tab_off : nullptr, (long long) (g.w.Z / size_t (lim_block)) };
          at_block (args.host (a_enc)[k], enc, lim_block);
        }
    }
  // the arguments at 44.1 kHz
  std::vector<long long> spans (nf);
  size_t staged = 0;
  for (size_t k = 0; k < nf; k++)
    {
      const FSeg& g = fgeo[k];
      const size_t i = at_44[k], s = segs[i];
      const float *in = ctx->ws_seg_in.as<float>() + g.stage_off;
      float *out = ctx->ws_seg_out.as<float>() + g.stage_off;
      if constexpr (!S16)
        if (!g.r)
          {
            in = pcm_in_d[s];
            out = out_d[s];
          }
      awmk::AddMixArgs a {};
      a.pcm_in = in;
      a.out = out;
      a.n_frames = (long long) g.len;
      a.n_channels = 2;
      a.frame_mod = table_of (i);
      fill_add_mix_common (a, params().water_delta);
      a.first_frame = (long long) (g.skipped / FRAME);
      a.block_max = use_limiter ? reinterpret_cast<unsigned int *> (block_max + g.max_off) : nullptr;
      a.first_block = (long long) g.first_block;
      a.n_blocks = (long long) g.n_blocks;
      a.frames_per_span = L_44;
      args.host (a_fmix)[k] = a;
      args.host (a_flim)[k] = { out, (long long) g.len, block_max + g.max_off, (long long) g.n_blocks, tabs + g.tab_off, (long long) g.n_tab,
                                (long long) g.skipped, (long long) g.first_block };
      spans[k] = ((long long) ((g.len + FRAME - 1) / FRAME) + L_44 - 1) / L_44;
      if (g.r || S16)
        {
          // (16-bit: `src` holds the address of the int16 values, launch_segment_gather_s16)
          args.host (a_gather)[staged] = { reinterpret_cast<const float *> (pcm_in_d[s]), ctx->ws_seg_in.as<float>() + g.stage_off,
                                           (long long) (n_frames[s] * 2), (long long) (g.r * 2) };
          if constexpr (S16)
            args.host (a_scatter)[staged] = { nullptr, out + g.r * 2, out_d[s], (long long) n_frames[s], (long long) zero_frames[s],
                                              use_limiter ? tabs + g.tab_off : nullptr, (long long) (g.skipped / LIMITER_BLOCK) };
          else
            args.host (a_scatter)[staged] = { out + g.r * 2, out_d[s], (long long) (n_frames[s] * 2), 0 };
          staged++;
        }
    }
  if (int rc = args.upload (ctx, st)) return rc;

  unsigned int ceiling_bits;
  std::memcpy (&ceiling_bits, &LIMITER_CEILING, sizeof (ceiling_bits));
  // one batch of the window kind: down, block maxima preset, K2 for the watermark alone, up, mix + maxima, limiter.  The `_rates`
  // launchers read the tables and the limiter block from the descriptors and check min_block; the one-rate launchers are given them
  auto run_rate_batch = [&] (const RBatch& b) -> int {
    const size_t nb = b.i1 - b.i0;
    double down_values = 0, up_values = 0, n44_values = 0, out_values = 0;
    long long max_spans = 0;
    size_t lds_down = 0, lds_up = 0;                       // (MIXED only)
    for (size_t q = b.d0; q < b.d1; q++)
      {
        down_values += double (slice_of (h_down[q]).n_in + slice_of (h_down[q]).n_out) * C;
        if constexpr (MIXED)
          lds_down = std::max (lds_down, awmk::resample_slice_lds_bytes (h_down[q]));
      }
    for (size_t k = b.i0; k < b.i1; k++)
      {
        up_values += double (slice_of (h_up[k]).n_in + slice_of (h_up[k]).n_out) * C;
        if constexpr (MIXED)
          lds_up = std::max (lds_up, awmk::resample_slice_lds_bytes (h_up[k]));
        n44_values += double (rgeo[k].w.slice_frames * FRAME) * C;
        out_values += double (rgeo[k].w.n) * C;
        max_spans = std::max (max_spans, ((long long) rgeo[k].w.slice_frames + L_rate - 1) / L_rate);
      }
    const RateTables& t = *rgeo[b.i0].t;                   // (!MIXED: the call's one rate)
    {
      ProfScope ps (ctx, PROF_RESAMPLE, down_values * 4.0, st);                     // every input and output sample once
      if constexpr (MIXED && S16)
        AWM_HIP_CHECK (awmk::launch_resample_slices_rates_s16 (st, d_down + b.d0, int (b.d1 - b.d0), C, (long long) b.max_n44, true, lds_down));
      else if constexpr (MIXED)
        AWM_HIP_CHECK (awmk::launch_resample_slices_rates (st, d_down + b.d0, int (b.d1 - b.d0), C, (long long) b.max_n44, true, lds_down));
      else if constexpr (S16)
        AWM_HIP_CHECK (awmk::launch_resample_slices_s16 (st, resample_table_args (*t.down, C), d_down + b.d0, int (b.d1 - b.d0), (long long) b.max_n44, true));
      else
        AWM_HIP_CHECK (awmk::launch_resample_slices (st, resample_table_args (*t.down, C), d_down + b.d0, int (b.d1 - b.d0), (long long) b.max_n44, true));
    }
    if (use_limiter)
      {
        const size_t m0 = rgeo[b.i0].max_off, m1 = rgeo[b.i1 - 1].max_off + size_t (rgeo[b.i1 - 1].w.p.n_blocks);
        AWM_HIP_CHECK (awmk::launch_fill_u32 (st, reinterpret_cast<unsigned int *> (block_max + m0), ceiling_bits, m1 - m0));
      }
    {
      ProfScope ps (ctx, PROF_ADD_MIX, n44_values * 8.0, st);
      AWM_HIP_CHECK (awmk::launch_add_mix_batch (st, ctx->tabs, d_rmix + b.i0, int (nb), max_spans, int (block_frames), int (Params::frames_pad_start)));
    }
    {
      ProfScope ps (ctx, PROF_RESAMPLE, up_values * 4.0, st);
      if constexpr (MIXED)
        AWM_HIP_CHECK (awmk::launch_resample_slices_rates (st, d_up + b.i0, int (nb), C, (long long) b.max_out, true, lds_up));
      else
        AWM_HIP_CHECK (awmk::launch_resample_slices (st, resample_table_args (*t.up, C), d_up + b.i0, int (nb), (long long) b.max_out, true));
    }
    if constexpr (S16)
      {
        // the block maxima from the mix, the ramp tables, then the mix again: limited, encoded and stored as int16
        if (use_limiter)
          {
            if constexpr (MIXED)
              {
                AWM_HIP_CHECK (awmk::launch_max_segments_rates_s16 (st, d_mm + b.i0, int (nb), (long long) b.max_out, C, b.min_block));
                AWM_HIP_CHECK (awmk::launch_limiter_table_batch_rates (st, d_rlim + b.i0, int (nb), LIMITER_CEILING, (long long) b.max_tab));
              }
            else
              {
                AWM_HIP_CHECK (awmk::launch_max_segments_s16 (st, d_mm + b.i0, int (nb), (long long) b.max_out, C, t.limiter_block));
                AWM_HIP_CHECK (awmk::launch_limiter_table_batch (st, d_rlim + b.i0, int (nb), (long long) b.max_len, t.limiter_block, LIMITER_CEILING,
                                                                 (long long) b.max_tab));
              }
          }
        ProfScope ps (ctx, PROF_LIMIT_ENCODE_S16, out_values * 8.0, st);            // int16 and float in, int16 out
        if constexpr (MIXED)
          AWM_HIP_CHECK (awmk::launch_limit_encode_segments_rates (st, d_enc + b.i0, int (nb), (long long) b.max_len, true, b.min_block));
        else
          AWM_HIP_CHECK (awmk::launch_limit_encode_segments (st, d_enc + b.i0, int (nb), (long long) b.max_len, true, t.limiter_block));
      }
    else
      {
        if constexpr (MIXED)
          AWM_HIP_CHECK (awmk::launch_mix_max_segments_rates (st, d_mm + b.i0, int (nb), (long long) b.max_out, C, b.min_block));
        else
          AWM_HIP_CHECK (awmk::launch_mix_max_segments (st, d_mm + b.i0, int (nb), (long long) b.max_out, C, t.limiter_block));
        if (use_limiter)
          {
            ProfScope ps (ctx, PROF_LIMITER, out_values * 8.0, st);
            if constexpr (MIXED)
              AWM_HIP_CHECK (awmk::launch_limiter_batch_rates (st, d_rlim + b.i0, int (nb), (long long) b.max_len, C, b.min_block, LIMITER_CEILING,
                                                               (long long) b.max_tab));
            else
              AWM_HIP_CHECK (awmk::launch_limiter_batch (st, d_rlim + b.i0, int (nb), (long long) b.max_len, C, t.limiter_block, LIMITER_CEILING,
                                                         (long long) b.max_tab));
          }
      }
    return 0;
  };
  // one batch at 44.1 kHz: gather, block maxima preset, K2, limiter (16-bit: its tables, then limit + encode), scatter
  auto run_44_batch = [&] (const FBatch& b) -> int {
    const size_t nb = b.i1 - b.i0;
    long long max_spans = 0;
    double values = 0;
    for (size_t k = b.i0; k < b.i1; k++)
      {
        max_spans = std::max (max_spans, spans[k]);
        values += double (fgeo[k].len) * 2;
      }
    if constexpr (S16)
      {
        ProfScope ps (ctx, PROF_SEGMENT_GATHER_S16, values * 6.0, st);            // int16 in, float out
        AWM_HIP_CHECK (awmk::launch_segment_gather_s16 (st, d_gather + b.g0, int (b.g1 - b.g0), (long long) b.max_len * 2));
      }
    else if (b.g1 > b.g0)
      AWM_HIP_CHECK (awmk::launch_segment_copy (st, d_gather + b.g0, int (b.g1 - b.g0), (long long) b.max_len * 2));
    if (use_limiter)
      {
        const size_t m0 = fgeo[b.i0].max_off, m1 = fgeo[b.i1 - 1].max_off + fgeo[b.i1 - 1].n_blocks;
        AWM_HIP_CHECK (awmk::launch_fill_u32 (st, reinterpret_cast<unsigned int *> (block_max + m0), ceiling_bits, m1 - m0));
      }
    {
      ProfScope ps (ctx, PROF_ADD_MIX, values * 8.0, st);                          // read + write every sample once
      AWM_HIP_CHECK (awmk::launch_add_mix_batch (st, ctx->tabs, d_fmix + b.i0, int (nb), max_spans, int (block_frames), int (Params::frames_pad_start)));
    }
    if constexpr (S16)
      {
        // the ramp tables alone, then limit + encode from the staged mix to the caller's buffers
        if (use_limiter)
          AWM_HIP_CHECK (awmk::launch_limiter_table_batch (st, d_flim + b.i0, int (nb), (long long) b.max_len, LIMITER_BLOCK, LIMITER_CEILING, (long long) b.max_tab));
        ProfScope ps (ctx, PROF_LIMIT_ENCODE_S16, values * 6.0, st);               // float in, int16 out
        AWM_HIP_CHECK (awmk::launch_limit_encode_segments (st, d_scatter + b.g0, int (b.g1 - b.g0), (long long) b.max_len, false, LIMITER_BLOCK));
      }
    else
      {
        if (use_limiter)
          {
            ProfScope ps (ctx, PROF_LIMITER, values * 8.0, st);
            AWM_HIP_CHECK (awmk::launch_limiter_batch (st, d_flim + b.i0, int (nb), (long long) b.max_len, 2, LIMITER_BLOCK, LIMITER_CEILING, (long long) b.max_tab));
          }
        if (b.g1 > b.g0)
          AWM_HIP_CHECK (awmk::launch_segment_copy (st, d_scatter + b.g0, int (b.g1 - b.g0), (long long) b.max_len * 2));
      }
    return 0;
  };

  // table group by table group: its tables once, then its batches of the window kind, then its batches at 44.1 kHz
  size_t rb = 0, fb = 0, group_built = size_t (-1);
  while (rb < rbatches.size() || fb < fbatches.size())
    {
      const size_t gr = rb < rbatches.size() ? group_of (at_rate[rbatches[rb].i0]) : size_t (-1);
      const size_t gf = fb < fbatches.size() ? group_of (at_44[fbatches[fb].i0]) : size_t (-1);
      const size_t group = std::min (gr, gf);
      if (group != group_built)
        {
          if (int rc = segment_table_group (ctx, st, tmpl, mk, group * TABLE_GROUP, std::min (TABLE_GROUP, n_distinct - group * TABLE_GROUP),
                                            args.dev (a_coded), n_code))
            return rc;
          group_built = group;
        }
      if (int rc = gr == group ? run_rate_batch (rbatches[rb++]) : run_44_batch (fbatches[fb++]))
        return rc;
    }
  return 0;
}

/* the ten entry points' body.  T = float or int16_t; per_key: keys + 16 i is the key of segment i, else keys is the one key;
 * per_segment: rates[i] is the rate of segment i, else rates[0] is the rate of the call.  What cannot take the fused path -- not stereo,
 * one segment, a pointer off the grid (16 bytes; 16-bit: a stereo frame), a limiter block below the batched limiter's floor, a window
 * beyond a workspace -- goes segment by segment, each at its rate; 16-bit through the definition itself: awm_pcm_decode_d into ws_seg_in,
 * the float path of one segment into ws_seg_out, awm_pcm_encode_d (direct16) into the caller's buffer */
template<class T> static int
add_segments_any (awm_ctx *ctx, const char *fn, const uint8_t *keys, bool per_key, size_t n_segments, const char *const *payload_hex,
                  const size_t *zero_frames, const T *const *pcm_in_d, T *const *out_d, const size_t *n_frames, int n_channels, const int *rates,
                  bool per_segment)
{
  constexpr bool S16 = std::is_same<T, int16_t>::value;
  AWM_ENTER (ctx);
  g_add_segments_fused_in_use = 0;
  if (per_segment)
    {
      if (!n_segments)
        return 0;
      if (!rates)
        {
          set_error (string_printf ("%s: sample_rates is null", fn));
          return AWM_ERR_ARG;
        }
    }
  auto rate_of = [&] (size_t i) { return rates[per_segment ? i : 0]; };
  std::map<int, RateTables> rate_tables;                     // the rates other than 44.1 kHz
  for (size_t i = 0; i < (per_segment ? n_segments : 1); i++)
    {
      const int rate = rate_of (i);
      awm_segment_plan probe;
      if (rate == Params::mark_sample_rate || rate_tables.count (rate))
        continue;
      if (awm_add_segment_plan (rate, 0, 0, &probe))
        {
          const std::string at = per_segment ? string_printf (" at index %zu", i) : std::string();
          set_error (rate <= 0 ? string_printf ("%s: bad sample rate %d%s", fn, rate, at.c_str())
                               : string_printf ("%s: no fixed-ratio resampler between %d Hz and %d Hz%s (zita's VResampler is not offered here)",
                                                fn, rate, Params::mark_sample_rate, at.c_str()));
          return AWM_ERR_ARG;
        }
      rate_tables[rate].limiter_block = int (probe.limiter_block);
    }
  if (!n_segments)
    return 0;
  std::vector<size_t> payload_index;
  std::vector<unsigned char> coded;
  size_t n_code = 0;
  if (int rc = segments_check (ctx, fn, keys, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels, payload_index, coded, n_code))
    return rc;
  for (size_t i = 0; i < n_segments; i++)
    {
      awm_segment_plan probe;
      if (rate_of (i) != Params::mark_sample_rate && awm_add_segment_plan (rate_of (i), zero_frames[i], n_frames[i], &probe))
        {
          set_error (string_printf ("%s: zero_frames + n_frames of segment %zu is not below 2^40", fn, i));
          return AWM_ERR_ARG;
        }
    }
  for (auto& rt : rate_tables)
    {
      rt.second.down = ctx->get_resample_table (rt.first, Params::mark_sample_rate);
      rt.second.up = ctx->get_resample_table (Params::mark_sample_rate, rt.first);
      if (!rt.second.down || !rt.second.up)
        return AWM_ERR_HIP;
    }
  if (per_key && segments_share_one_key (keys, n_segments))      // one key for all segments IS the one-key call
    per_key = false;
  // the fused path: stereo, the pointers on the grid, at every other rate the floor of the batched limiter (blocks of at least four of
  // its runs: launch_limiter_batch) and windows that fit the workspaces
  bool fused = g_add_batched && n_channels == 2 && n_segments >= 2;
  for (const auto& rt : rate_tables)
    fused = fused && rt.second.limiter_block >= 8192;
  for (size_t i = 0; i < n_segments && fused; i++)
    if (n_frames[i])
      {
        if ((reinterpret_cast<uintptr_t> (pcm_in_d[i]) | reinterpret_cast<uintptr_t> (out_d[i])) & (S16 ? 3 : 15))
          fused = false;
        else if (rate_of (i) != Params::mark_sample_rate)
          fused = segments_rate_fit_the_workspaces (1, zero_frames + i, n_frames + i, n_channels, rate_of (i));
      }
  if (!fused)
    {
      const RateTables *one_rate = rate_tables.empty() ? nullptr : &rate_tables.begin()->second;
      for (size_t i = 0; i < n_segments; i++)
        if (n_frames[i])
          {
            const uint8_t *key = per_key ? keys + 16 * i : keys;
            const int rate = rate_of (i);
            const RateTables *rt = rate == Params::mark_sample_rate ? nullptr : per_segment ? &rate_tables.at (rate) : one_rate;
            auto one = [&] (const float *in, float *out) {
              return rt ? add_segment_rate (ctx, *rt->down, *rt->up, key, payload_hex[i], zero_frames[i], in, out, n_frames[i], n_channels, rate)
                        : add_segment_stream (ctx, key, payload_hex[i], zero_frames[i], in, out, n_frames[i], n_channels);
            };
            if constexpr (S16)
              {
                const size_t n_values = n_frames[i] * size_t (n_channels);
                if (int rc = ctx->ws_seg_in.reserve (n_values * sizeof (float))) return rc;
                if (int rc = ctx->ws_seg_out.reserve (n_values * sizeof (float))) return rc;
                float *f = ctx->ws_seg_in.as<float>(), *g = ctx->ws_seg_out.as<float>();
                if (int rc = awm_pcm_decode_d (ctx, pcm_in_d[i], n_values, 16, 0, 0, f)) return rc;
                if (int rc = one (f, g)) return rc;
                if (int rc = awm_pcm_encode_d (ctx, g, n_values, 16, 0, 0, 1, out_d[i])) return rc;
              }
            else if (int rc = one (pcm_in_d[i], out_d[i]))
              return rc;
          }
      return 0;
    }
  SegmentKeys mk;
  std::vector<size_t> segs, table_of;
  std::vector<unsigned char> coded_tables;
  if (per_key)
    segments_by_key_and_payload (n_segments, keys, n_frames, payload_index, coded, n_code, mk, segs, table_of, coded_tables);
  else
    segments_by_payload (n_segments, n_frames, payload_index, segs, table_of);
  g_add_segments_fused_in_use = 1;
  if (segs.empty())
    return 0;
  auto *fused_fn = per_segment ? add_segments_fused<T, true> : add_segments_fused<T, false>;
  return fused_fn (ctx, rate_tables, per_key ? nullptr : keys, segs, table_of, per_key ? coded_tables : coded, n_code, zero_frames, pcm_in_d, out_d,
                   n_frames, rates, per_key ? &mk : nullptr);
}
} // extern "C++"

/* the entry points: which of them a call IS -- all rates equal: the one-rate function, 44.1 kHz: the function without a rate, one key for
 * all: the one-key function -- is decided here, before anything else happens; the messages of a call carry that function's name */
static const int RATE_44100 = Params::mark_sample_rate;

int
awm_add_watermark_segments_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                              const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames, int n_channels)
{
  return add_segments_any (ctx, "awm_add_watermark_segments_d", key, false, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels,
                           &RATE_44100, false);
}

int
awm_add_watermark_segments_rate_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                                   const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames, int n_channels, int sample_rate)
{
  if (sample_rate == Params::mark_sample_rate)
    return awm_add_watermark_segments_d (ctx, key, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels);
  return add_segments_any (ctx, "awm_add_watermark_segments_rate_d", key, false, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames,
                           n_channels, &sample_rate, false);
}

int
awm_add_watermark_segments_keys_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                                   const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames, int n_channels)
{
  if (ctx && keys && n_segments && segments_share_one_key (keys, n_segments))
    return awm_add_watermark_segments_d (ctx, keys, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels);
  return add_segments_any (ctx, "awm_add_watermark_segments_keys_d", keys, true, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames,
                           n_channels, &RATE_44100, false);
}

int
awm_add_watermark_segments_keys_rate_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                                        const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames, int n_channels, int sample_rate)
{
  if (sample_rate == Params::mark_sample_rate)
    return awm_add_watermark_segments_keys_d (ctx, keys, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels);
  if (ctx && keys && n_segments && segments_share_one_key (keys, n_segments))
    return awm_add_watermark_segments_rate_d (ctx, keys, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels, sample_rate);
  return add_segments_any (ctx, "awm_add_watermark_segments_keys_rate_d", keys, true, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames,
                           n_channels, &sample_rate, false);
}

int
awm_add_watermark_segments_rate_s16_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                                       const int16_t *const *pcm_in_d, int16_t *const *out_d, const size_t *n_frames, int n_channels, int sample_rate)
{
  return add_segments_any (ctx, "awm_add_watermark_segments_rate_s16_d", key, false, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames,
                           n_channels, &sample_rate, false);
}

int
awm_add_watermark_segments_keys_rate_s16_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                                            const int16_t *const *pcm_in_d, int16_t *const *out_d, const size_t *n_frames, int n_channels, int sample_rate)
{
  return add_segments_any (ctx, "awm_add_watermark_segments_keys_rate_s16_d", keys, true, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames,
                           n_channels, &sample_rate, false);
}

int
awm_add_watermark_segments_rates_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                                    const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames, int n_channels, const int *sample_rates)
{
  if (rates_all_equal (n_segments, sample_rates))
    return awm_add_watermark_segments_rate_d (ctx, key, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels, sample_rates[0]);
  return add_segments_any (ctx, "awm_add_watermark_segments_rates_d", key, false, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames,
                           n_channels, sample_rates, true);
}

int
awm_add_watermark_segments_keys_rates_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                                         const float *const *pcm_in_d, float *const *out_d, const size_t *n_frames, int n_channels, const int *sample_rates)
{
  if (rates_all_equal (n_segments, sample_rates))
    return awm_add_watermark_segments_keys_rate_d (ctx, keys, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels, sample_rates[0]);
  return add_segments_any (ctx, "awm_add_watermark_segments_keys_rates_d", keys, true, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames,
                           n_channels, sample_rates, true);
}

// (16-bit: sample_rates may be null -- every segment at 44.1 kHz, like awm_get_watermark_batch_rates_s16_d)
int
awm_add_watermark_segments_rates_s16_d (awm_ctx *ctx, const uint8_t key[16], size_t n_segments, const char *const *payload_hex, const size_t *zero_frames,
                                        const int16_t *const *pcm_in_d, int16_t *const *out_d, const size_t *n_frames, int n_channels, const int *sample_rates)
{
  if (!sample_rates || rates_all_equal (n_segments, sample_rates))
    return awm_add_watermark_segments_rate_s16_d (ctx, key, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels,
                                                  sample_rates ? sample_rates[0] : int (Params::mark_sample_rate));
  return add_segments_any (ctx, "awm_add_watermark_segments_rates_s16_d", key, false, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames,
                           n_channels, sample_rates, true);
}

int
awm_add_watermark_segments_keys_rates_s16_d (awm_ctx *ctx, const uint8_t *keys, size_t n_segments, const char *const *payload_hex,
                                             const size_t *zero_frames, const int16_t *const *pcm_in_d, int16_t *const *out_d, const size_t *n_frames,
                                             int n_channels, const int *sample_rates)
{
  if (!sample_rates || rates_all_equal (n_segments, sample_rates))
    return awm_add_watermark_segments_keys_rate_s16_d (ctx, keys, n_segments, payload_hex, zero_frames, pcm_in_d, out_d, n_frames, n_channels,
                                                       sample_rates ? sample_rates[0] : int (Params::mark_sample_rate));
  return add_segments_any (ctx, "awm_add_watermark_segments_keys_rates_s16_d", keys, true, n_segments, payload_hex, zero_frames, pcm_in_d, out_d,
                           n_frames, n_channels, sample_rates, true);
}

/* K16t alone (measurements, tests): the templates of n_keys keys built on the device, KEY_TMPL_LAUNCH per launch, and copied to the host,
 * n_keys x awmk::payload_table_stride (2226) entries -- they must equal awm_tab_frame_mod_template key by key, zeros behind.  out may be
 * NULL: the launches alone, on the context's stream (for timing) */
int
awm_debug_key_templates_d (awm_ctx *ctx, const uint8_t *keys, size_t n_keys, int16_t *out)
{
  AWM_ENTER (ctx);
  if (!keys || !n_keys || !key_templates_on_device_possible())
    {
      set_error ("awm_debug_key_templates_d: bad argument (keys; the default geometry: mix, two frames per bit, 128 payload bits)");
      return AWM_ERR_ARG;
    }
  const size_t stride = awmk::payload_table_stride (mark_block_frame_count());
  if (int rc = ctx->ws_keytab_aux.reserve (keytab_aux_layout (KEY_TMPL_LAUNCH, false).bytes)) return rc;
  std::vector<char> args;
  for (size_t g0 = 0; g0 < n_keys; g0 += KEY_TMPL_LAUNCH)
    {
      // a launch window of keys through the segments' own staging and launch (no tables: tmpl_of stays empty)
      const size_t gn = std::min (KEY_TMPL_LAUNCH, n_keys - g0);
      SegmentKeys mk;
      for (size_t i = 0; i < gn; i++)
        {
          mk.keys.emplace_back();
          std::memcpy (mk.keys.back().data(), keys + 16 * (g0 + i), 16);
        }
      if (int rc = mk.reserve (ctx, stride, true)) return rc;
      args.resize (mk.arg_bytes());
      mk.fill (args.data(), ctx->ws_keytab_aux.as<char>());
      AWM_HIP_CHECK (hipMemcpyAsync (ctx->ws_keytab_aux.ptr, args.data(), args.size(), hipMemcpyHostToDevice, ctx->stream));
      if (int rc = mk.build (ctx, ctx->stream, gn)) return rc;
      if (out)
        AWM_HIP_CHECK (hipMemcpyAsync (out + g0 * stride, ctx->ws_key_tmpl.ptr, gn * stride * sizeof (int16_t), hipMemcpyDeviceToHost, ctx->stream));
      AWM_HIP_CHECK (stream_wait (ctx->stream));              // (the staging vector is refilled for the next launch)
    }
  return 0;
}

/* K16t + K16p (tests): the tables of n (key, payload) pairs, pair i with keys + 16 i, built on the device and copied to the host,
 * n x [2][2226][81] bytes -- they must equal awm_tab_frame_mod (key i, payload i) */
int
awm_debug_key_payload_tables_d (awm_ctx *ctx, const uint8_t *keys, const char *const *payload_hex, size_t n, int8_t *tables_out)
{
  AWM_ENTER (ctx);
  if (!keys || !payload_hex || !tables_out || !n || n > 1024 || !key_templates_on_device_possible())
    {
      set_error ("awm_debug_key_payload_tables_d: bad argument (1 .. 1024 pairs; the default geometry: mix, two frames per bit, 128 payload bits)");
      return AWM_ERR_ARG;
    }
  const size_t n_code = code_size (ConvBlockType::a, params().payload_size), block_frames = mark_block_frame_count();
  const size_t table_stride = awmk::payload_table_stride (block_frames), table_bytes = 2 * block_frames * Params::n_bands;
  // the pairs by key (K16p's tables are ordered by template); pair order[t] becomes table t
  std::vector<size_t> order (n);
  for (size_t i = 0; i < n; i++)
    order[i] = i;
  std::stable_sort (order.begin(), order.end(), [&] (size_t x, size_t y) { return std::memcmp (keys + 16 * x, keys + 16 * y, 16) < 0; });
  SegmentKeys mk;
  std::vector<unsigned char> coded;
  for (size_t t = 0; t < n; t++)
    {
      const size_t p = order[t];
      const std::vector<int> bits = parse_payload (payload_hex[p] ? payload_hex[p] : "");
      if (bits.empty())
        {
          set_error (string_printf ("awm_debug_key_payload_tables_d: cannot parse the payload at index %zu", p));
          return AWM_ERR_ARG;
        }
      if (int rc = payload_code_append (bits, n_code, coded)) return rc;
      if (!t || std::memcmp (keys + 16 * p, keys + 16 * order[t - 1], 16))
        {
          mk.keys.emplace_back();
          std::memcpy (mk.keys.back().data(), keys + 16 * p, 16);
        }
      mk.key_of_table.push_back (int (mk.keys.size() - 1));
    }
  if (int rc = mk.reserve (ctx, table_stride)) return rc;
  const size_t off_keys = (coded.size() + 15) / 16 * 16;
  std::vector<char> args (off_keys + mk.arg_bytes());
  std::memcpy (args.data(), coded.data(), coded.size());
  if (int rc = ctx->ws_keytab.reserve (n * table_stride)) return rc;
  if (int rc = ctx->ws_keytab_aux.reserve (args.size())) return rc;
  mk.fill (args.data() + off_keys, ctx->ws_keytab_aux.as<char>() + off_keys);
  if (int rc = upload_sync (ctx->ws_keytab_aux, args.data(), args.size(), ctx->stream)) return rc;
  if (int rc = segment_table_group (ctx, ctx->stream, nullptr, &mk, 0, n, ctx->ws_keytab_aux.as<unsigned char>(), n_code)) return rc;
  for (size_t t = 0; t < n; t++)
    AWM_HIP_CHECK (hipMemcpyAsync (tables_out + order[t] * table_bytes, ctx->ws_keytab.as<int8_t>() + t * table_stride, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
  AWM_HIP_CHECK (stream_wait (ctx->stream));
  return 0;
}

/* K16p alone (measurements, tests): the tables of n_payloads payloads with one key built on the device and copied to the host,
 * n_payloads x [2][block frames][81] bytes -- they must equal awm_tab_frame_mod payload by payload.  tables_out may be NULL: the launch
 * alone, on the context's stream (for timing) */
int
awm_debug_payload_tables_d (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads, int8_t *tables_out)
{
  AWM_ENTER (ctx);
  if (!key || !payload_hex || !n_payloads || n_payloads > 1024)
    {
      set_error ("awm_debug_payload_tables_d: bad argument (1 .. 1024 payloads)");
      return AWM_ERR_ARG;
    }
  const size_t n_code = code_size (ConvBlockType::a, params().payload_size), block_frames = mark_block_frame_count();
  const size_t table_stride = awmk::payload_table_stride (block_frames), table_bytes = 2 * block_frames * Params::n_bands;
  std::vector<unsigned char> coded;
  for (size_t p = 0; p < n_payloads; p++)
    {
      const std::vector<int> bits = parse_payload (payload_hex[p] ? payload_hex[p] : "");
      if (bits.empty())
        {
          set_error (string_printf ("awm_debug_payload_tables_d: cannot parse the payload at index %zu", p));
          return AWM_ERR_ARG;
        }
      if (int rc = payload_code_append (bits, n_code, coded)) return rc;
    }
  FrameModTemplate *tmpl = ctx->get_frame_mod_template (capi_key (key));
  if (!tmpl)
    return AWM_ERR_HIP;
  if (int rc = ctx->ws_keytab.reserve (n_payloads * table_stride)) return rc;
  if (int rc = upload_sync (ctx->ws_keytab_aux, coded.data(), coded.size(), ctx->stream)) return rc;
  if (int rc = segment_table_group (ctx, ctx->stream, tmpl, nullptr, 0, n_payloads, ctx->ws_keytab_aux.as<unsigned char>(), n_code)) return rc;
  if (tables_out)
    {
      AWM_HIP_CHECK (hipMemcpy2DAsync (tables_out, table_bytes, ctx->ws_keytab.ptr, table_stride, table_bytes, n_payloads, hipMemcpyDeviceToHost, ctx->stream));
      AWM_HIP_CHECK (stream_wait (ctx->stream));
    }
  return 0;
}

/* the same with ONE KEY PER CLIP (BASELINE configs[4]: `--test-key k` per clip).  The frame_mod tables (361 KB per key; 2226 up / down
 * draws and three shuffles per key on the host: ~3 ms of one core) are built on host threads group by group while the device works on
 * the previous group, and live in one batch buffer instead of the context's per-key cache. */
/* (measurement knob) 1 (default): the frame_mod tables of a batch with one key per clip are built on the device (K16, hip/keytab.hip) |
 * 0: on host threads */
extern "C" void awm_debug_set_key_tables_on_device (int on) { g_key_tables_on_device = on; }

constexpr size_t KEY_TABLE_LAUNCH = 256;       // keys per launch of K16: one workgroup = one compute unit per key

/* K16's block for the keys of a batch of clips with one payload (keytab_stage.hh): one page-locked block (pin_keytab), one upload to
 * ws_keytab_aux on st.  The block is the context's: the caller waits for the upload before it returns */
static int
clip_keys_aux_upload (awm_ctx *ctx, hipStream_t st, const uint8_t *keys, size_t n_keys, const std::vector<int>& bits, KeytabAux& aux)
{
  std::vector<unsigned char> coded;
  if (int rc = payload_code_append (bits, KEYTAB_CODE_BITS, coded)) return rc;
  const size_t aux_bytes = keytab_aux_layout (n_keys, true).bytes;
  if (int rc = ctx->pin_keytab.reserve (aux_bytes)) return rc;
  if (int rc = ctx->ws_keytab_aux.reserve (aux_bytes)) return rc;
  aux = keytab_aux_pack (ctx->pin_keytab.as<unsigned char>(), n_keys, keys, coded.data());
  AWM_HIP_CHECK (hipMemcpyAsync (ctx->ws_keytab_aux.ptr, ctx->pin_keytab.ptr, aux_bytes, hipMemcpyHostToDevice, st));
  return 0;
}

/* K16 for keys first_key .. first_key + n_keys - 1 of the block in ws_keytab_aux, KEY_TABLE_LAUNCH per launch on st (the launches of a
 * stream share ws_keytab_scratch): their tables from `tables` on, one behind the other */
static int
key_tables_run (awm_ctx *ctx, hipStream_t st, const KeytabAux& aux, size_t first_key, size_t n_keys, int8_t *tables)
{
  const size_t table_bytes = awmk::key_table_bytes();
  for (size_t g0 = 0; g0 < n_keys; g0 += KEY_TABLE_LAUNCH)
    {
      const size_t gn = std::min (KEY_TABLE_LAUNCH, n_keys - g0);
      awmk::KeyTableArgs ka = keytab_args (ctx->ws_keytab_aux.as<unsigned char>(), aux, first_key + g0, gn,
                                           ctx->ws_keytab_scratch.as<unsigned char>(), KEY_TABLE_LAUNCH);
      ka.tables = reinterpret_cast<signed char *> (tables + g0 * table_bytes);
      ProfScope ps (ctx, PROF_KEYTAB, double (gn) * table_bytes, st);                  // the table out, once (360 KB per key)
      AWM_HIP_CHECK (awmk::launch_frame_mod_tables (st, ka));
    }
  return 0;
}

/* Batched clips with a key per clip, everything on the context's stream: FIRST the tables of (up to 4096) keys, 256 per launch of K16, THEN the
 * clips in one launch per stage.  K16 holds 116 KB of LDS on every compute unit it runs on: beside it K2 runs one workgroup per unit
 * instead of four, and the first group's tables are waited for in any case -- building the next group's tables WHILE a group is
 * watermarked (add_batch_keys_device_tables below, awm_debug_set_add_batched (1)) cost more than it hid once the clips of a group took 3 ms instead of 8. */
static int
add_batch_keys_tables_first (awm_ctx *ctx, const uint8_t *keys, const std::vector<int>& bits, size_t n_clips, const float *const *pcm_in_d,
                             float *const *out_d, const size_t *n_frames)
{
  constexpr size_t SUPER = 4096;
  const size_t table_bytes = awmk::key_table_bytes();
  const int use_limiter = !params().test_no_limiter;
  hipStream_t st = ctx->stream;
  if (int rc = ctx->ws_keytab.reserve (std::min (n_clips, SUPER) * table_bytes)) return rc;
  if (int rc = ctx->ws_keytab_scratch.reserve (KEY_TABLE_LAUNCH * awmk::key_table_scratch_bytes())) return rc;
  KeytabAux aux;
  if (int rc = clip_keys_aux_upload (ctx, st, keys, n_clips, bits, aux)) return rc;
  Events ev_aux;
  if (int rc = ev_aux.create (1)) return rc;
  AWM_HIP_CHECK (hipEventRecord (ev_aux[0], st));
  std::vector<const int8_t *> tables (n_clips);
  for (size_t i = 0; i < n_clips; i++)
    tables[i] = ctx->ws_keytab.as<int8_t>() + (i % SUPER) * table_bytes;
  AddBatchArgs batch;
  if (int rc = add_batch_stage (ctx, st, n_clips, pcm_in_d, out_d, n_frames, tables, use_limiter, batch))
    return rc;
  for (size_t s0 = 0; s0 < n_clips; s0 += SUPER)
    {
      const size_t sn = std::min (SUPER, n_clips - s0);
      if (int rc = key_tables_run (ctx, st, aux, s0, sn, ctx->ws_keytab.as<int8_t>()))
        return rc;
      if (int rc = add_batch_run (ctx, st, batch, s0, sn, use_limiter))
        return rc;
    }
  // (the staging block is the context's: its upload has to be through before the next call refills it)
  AWM_HIP_CHECK (hipEventSynchronize (ev_aux[0]));
  return 0;
}

/* awm_add_watermark_batch_keys_d with the tables built by K16: groups of GROUP keys (one workgroup = one compute unit per key), two
 * table areas in turn -- the tables of group g + 1 are built (on a lane of their own) while the clips of group g are watermarked on the
 * add lanes; what the host contributes per key is the AES key schedule (176 bytes). */
static int
add_batch_keys_device_tables (awm_ctx *ctx, const uint8_t *keys, const std::vector<int>& bits, size_t n_clips, const float *const *pcm_in_d,
                              float *const *out_d, const size_t *n_frames, int n_channels)
{
  constexpr size_t GROUP = KEY_TABLE_LAUNCH;               // (a group's tables are one launch)
  constexpr int ADD_LANES = 8;
  const size_t table_bytes = awmk::key_table_bytes();
  // a group of clips in one launch per stage on the context's stream (add_clips_batched above), or clip by clip on eight lanes
  const bool batched = add_clips_batchable (ctx, n_clips, pcm_in_d, out_d, n_channels);
  if (batched && g_add_batched == 2)
    return add_batch_keys_tables_first (ctx, keys, bits, n_clips, pcm_in_d, out_d, n_frames);
  const int use_limiter = !params().test_no_limiter;
  const int n_lanes = batched ? 1 : int (std::min<size_t> (ADD_LANES, n_clips));
  std::vector<WorkLane *> lanes;                           // lanes 0 .. n_lanes - 1 watermark, lane n_lanes builds tables
  if (int rc = lanes_with_sync (ctx, n_lanes + 1, lanes)) return rc;
  hipStream_t table_stream = lanes[n_lanes]->stream;
  if (int rc = ctx->ws_keytab.reserve (2 * GROUP * table_bytes)) return rc;
  if (int rc = ctx->ws_keytab_scratch.reserve (KEY_TABLE_LAUNCH * awmk::key_table_scratch_bytes())) return rc;
  KeytabAux aux;
  if (int rc = clip_keys_aux_upload (ctx, ctx->stream, keys, n_clips, bits, aux)) return rc;
  Events ev_aux, ev_tab, lane_done;                        // lane_done: [half][lane], the lane is through the clips of that half
  if (int rc = ev_aux.create (1)) return rc;
  if (int rc = ev_tab.create (2)) return rc;
  if (int rc = lane_done.create (2 * size_t (n_lanes))) return rc;
  AddBatchArgs batch;
  if (batched)
    {
      // clip i of group g finds its table in area g mod 2, slot i of the group
      std::vector<const int8_t *> tables (n_clips);
      for (size_t i = 0; i < n_clips; i++)
        tables[i] = ctx->ws_keytab.as<int8_t>() + (((i / GROUP) & 1) * GROUP + i % GROUP) * table_bytes;
      if (int rc = add_batch_stage (ctx, ctx->stream, n_clips, pcm_in_d, out_d, n_frames, tables, use_limiter, batch))
        return rc;
    }
  AWM_HIP_CHECK (hipEventRecord (ev_aux[0], ctx->stream)); // (also orders everything behind the clips' producers on the context's stream)
  AWM_HIP_CHECK (hipStreamWaitEvent (table_stream, ev_aux[0], 0));
  for (int i = 1; i < n_lanes; i++)
    AWM_HIP_CHECK (hipStreamWaitEvent (lanes[i]->stream, ev_aux[0], 0));
  int rc = 0;
  for (size_t g0 = 0, gi = 0; g0 < n_clips && !rc; g0 += GROUP, gi++)
    {
      const size_t gn = std::min (GROUP, n_clips - g0);
      const int half = int (gi & 1);
      int8_t *dev = ctx->ws_keytab.as<int8_t>() + size_t (half) * GROUP * table_bytes;
      if (gi >= 2)                                          // the clips of group gi - 2 (same table area) are through on every lane
        for (int i = 0; i < n_lanes; i++)
          AWM_HIP_CHECK (hipStreamWaitEvent (table_stream, lane_done[size_t (half) * n_lanes + i], 0));
      if (int rc_tab = key_tables_run (ctx, table_stream, aux, g0, gn, dev))
        return rc_tab;
      AWM_HIP_CHECK (hipEventRecord (ev_tab[half], table_stream));
      for (int i = 0; i < n_lanes; i++)
        AWM_HIP_CHECK (hipStreamWaitEvent (lanes[i]->stream, ev_tab[half], 0));
      if (batched)
        rc = add_batch_run (ctx, ctx->stream, batch, g0, gn, use_limiter);
      for (size_t i = 0; i < gn && !rc && !batched; i++)
        rc = add_full (ctx, pcm_in_d[g0 + i], out_d[g0 + i], n_frames[g0 + i], n_channels, dev + i * table_bytes, params().water_delta,
                       use_limiter, lanes[(g0 + i) % n_lanes]);
      for (int i = 0; i < n_lanes && !rc; i++)
        AWM_HIP_CHECK (hipEventRecord (lane_done[size_t (half) * n_lanes + i], lanes[i]->stream));
    }
  for (int i = 1; i < n_lanes; i++)
    {
      AWM_HIP_CHECK (hipEventRecord (lanes[i]->ev_sync, lanes[i]->stream));
      AWM_HIP_CHECK (hipStreamWaitEvent (ctx->stream, lanes[i]->ev_sync, 0));
    }
  AWM_HIP_CHECK (hipEventRecord (lanes[n_lanes]->ev_sync, table_stream));
  AWM_HIP_CHECK (hipStreamWaitEvent (ctx->stream, lanes[n_lanes]->ev_sync, 0));
  // (the staging block is the context's: its upload has to be through before the next call refills it)
  AWM_HIP_CHECK (hipEventSynchronize (ev_aux[0]));
  return rc;
}

/* the tables K16 builds, copied to the host: n_keys x 2 x 2226 x 81 bytes (for tests: they must equal awm_tab_frame_mod key by key) */
int
awm_debug_frame_mod_tables_d (awm_ctx *ctx, const uint8_t *keys, size_t n_keys, const char *payload_hex, int8_t *tables_out)
{
  AWM_ENTER (ctx);
  const std::vector<int> bits = parse_payload (payload_hex ? payload_hex : "");
  if (bits.empty() || !keys || !tables_out || !params().mix || code_size (ConvBlockType::a, params().payload_size) != KEYTAB_CODE_BITS)
    {
      set_error ("awm_debug_frame_mod_tables_d: bad argument");
      return AWM_ERR_ARG;
    }
  // a launch of keys at a time through the staging and the launches of the clip batches, into one table area
  const size_t table_bytes = awmk::key_table_bytes();
  if (int rc = ctx->ws_keytab.reserve (KEY_TABLE_LAUNCH * table_bytes)) return rc;
  if (int rc = ctx->ws_keytab_scratch.reserve (KEY_TABLE_LAUNCH * awmk::key_table_scratch_bytes())) return rc;
  for (size_t g0 = 0; g0 < n_keys; g0 += KEY_TABLE_LAUNCH)
    {
      const size_t gn = std::min (KEY_TABLE_LAUNCH, n_keys - g0);
      KeytabAux aux;
      if (int rc = clip_keys_aux_upload (ctx, ctx->stream, keys + 16 * g0, gn, bits, aux)) return rc;
      if (int rc = key_tables_run (ctx, ctx->stream, aux, 0, gn, ctx->ws_keytab.as<int8_t>())) return rc;
      AWM_HIP_CHECK (hipMemcpyAsync (tables_out + g0 * table_bytes, ctx->ws_keytab.ptr, gn * table_bytes, hipMemcpyDeviceToHost, ctx->stream));
      AWM_HIP_CHECK (stream_wait (ctx->stream));              // (the staging block and the table area are refilled for the next launch)
    }
  return 0;
}

int
awm_debug_clip_key_tables_check_d (awm_ctx *ctx, const uint8_t *keys, size_t n_keys, long long mismatch_out[9])
{
  AWM_ENTER (ctx);
  return clip_key_tables_check (ctx, keys, n_keys, mismatch_out);
}

int
awm_add_watermark_batch_keys_d (awm_ctx *ctx, const uint8_t *keys, const char *payload_hex, size_t n_clips, const float *const *pcm_in_d,
                                float *const *out_d, const size_t *n_frames, int n_channels)
{
  AWM_ENTER (ctx);
  if (n_clips && (!keys || !pcm_in_d || !out_d || !n_frames || n_channels < 1))
    {
      set_error ("awm_add_watermark_batch_keys_d: bad argument");
      return AWM_ERR_ARG;
    }
  const std::vector<int> bits = parse_payload (payload_hex ? payload_hex : "");
  if (bits.empty())
    {
      set_error (std::string ("cannot parse payload '") + (payload_hex ? payload_hex : "") + "'");
      return AWM_ERR_ARG;
    }
  const size_t table_bytes = 2 * mark_block_frame_count() * Params::n_bands;
  if (g_key_tables_on_device && params().mix && table_bytes == awmk::key_table_bytes()
      && code_size (ConvBlockType::a, params().payload_size) == KEYTAB_CODE_BITS && n_clips)
    return add_batch_keys_device_tables (ctx, keys, bits, n_clips, pcm_in_d, out_d, n_frames, n_channels);
  // The host path (--linear, or the device path switched off): a key's table costs about a millisecond of one host core and is 360 KB; the device needs 25 us per clip.  So the tables are built
  // for SUPER clips at a time on up to 64 host threads, straight into one half of a page-locked staging block (the workers copy,
  // not the launching thread), go to the device in ONE copy per SUPER, and the next SUPER is built while the device works on this one.
  // (Round 3a: one task per group of 64 with the launching thread copying 23 MB per group into the staging block: 90 ms for 1024
  // clips where the device needs 25.)
  constexpr size_t SUPER = 128;
  constexpr int ADD_LANES = 8;
  // device side: TWO halves of SUPER tables, like the staging block -- the size does not grow with the batch.  Half h is refilled
  // (super s, s >= 2) only after every lane has finished the clips of super s - 2: the upload waits for the lanes' events on the device.
  if (int rc = ctx->ws_keytab.reserve (2 * SUPER * table_bytes)) return rc;
  if (int rc = ctx->pin_keytab.reserve (2 * SUPER * table_bytes)) return rc;
  const int n_lanes = int (std::min<size_t> (ADD_LANES, std::max<size_t> (1, n_clips)));
  std::vector<WorkLane *> lanes;
  if (int rc = lanes_with_sync (ctx, n_lanes, lanes)) return rc;
  const std::vector<Key> key_list = key_list_from (keys, int (n_clips));
  ParamValues *const pv = &params();
  char *const pin_base = ctx->pin_keytab.as<char>();
  auto build_super = [&, pv] (size_t s0, int half) -> bool {
    const size_t sn = std::min (SUPER, n_clips - s0);
    char *pin = pin_base + size_t (half) * SUPER * table_bytes;
    const size_t n_threads = std::max<size_t> (1, std::min<size_t> ({ sn, size_t (64), size_t (std::max (1u, std::thread::hardware_concurrency())) }));
    std::atomic<size_t> next { 0 };
    std::atomic<bool> good { true };
    auto work = [&] {
      ParamsBind bind (pv);
      for (size_t i = next.fetch_add (1); i < sn; i = next.fetch_add (1))
        {
          const std::vector<int8_t> table = build_frame_mod_table (key_list[s0 + i], bits);
          if (table.size() != table_bytes)
            good = false;
          else
            std::memcpy (pin + i * table_bytes, table.data(), table_bytes);
        }
    };
    std::vector<std::thread> threads;
    for (size_t t = 1; t < n_threads; t++)
      threads.emplace_back (work);
    work();
    for (auto& t : threads)
      t.join();
    return good;
  };
  Events ev_up, lane_done;                                 // lane_done: [half][lane], the lane is through the clips of that half
  if (int rc = ev_up.create (2)) return rc;
  if (int rc = lane_done.create (2 * size_t (n_lanes))) return rc;
  int rc = 0, last_half = -1;
  std::future<bool> next_built;
  struct FutureGuard { std::future<bool>& f; ~FutureGuard() { if (f.valid()) f.wait(); } } future_guard { next_built };     // (the task writes into the staging block)
  for (size_t s0 = 0, sidx = 0; s0 < n_clips && !rc; s0 += SUPER, sidx++)
    {
      const size_t sn = std::min (SUPER, n_clips - s0);
      const int half = int (sidx & 1);
      const bool built = next_built.valid() ? next_built.get() : build_super (s0, half);
      if (!built)
        {
          set_error ("frame_mod table of unexpected size");
          return AWM_ERR_GENERIC;
        }
      if (s0 + SUPER < n_clips)
        {
          if (sidx >= 1)
            AWM_HIP_CHECK (hipEventSynchronize (ev_up[half ^ 1]));                      // the upload out of the other half is done
          next_built = std::async (std::launch::async, build_super, s0 + SUPER, half ^ 1);     // while the device works on this one
        }
      int8_t *dev = ctx->ws_keytab.as<int8_t>() + size_t (half) * SUPER * table_bytes;
      if (sidx >= 2)
        for (int i = 1; i < n_lanes; i++)                                               // (lane 0 is ctx->stream itself)
          AWM_HIP_CHECK (hipStreamWaitEvent (ctx->stream, lane_done[size_t (half) * n_lanes + i], 0));
      AWM_HIP_CHECK (hipMemcpyAsync (dev, pin_base + size_t (half) * SUPER * table_bytes, sn * table_bytes, hipMemcpyHostToDevice, ctx->stream));
      AWM_HIP_CHECK (hipEventRecord (ev_up[half], ctx->stream));
      for (int i = 1; i < n_lanes; i++)
        AWM_HIP_CHECK (hipStreamWaitEvent (lanes[i]->stream, ev_up[half], 0));          // (also orders the lanes after the clips' producers)
      for (size_t i = 0; i < sn && !rc; i++)
        rc = add_full (ctx, pcm_in_d[s0 + i], out_d[s0 + i], n_frames[s0 + i], n_channels, dev + i * table_bytes, params().water_delta,
                       !params().test_no_limiter, lanes[(s0 + i) % n_lanes]);
      for (int i = 1; i < n_lanes && !rc; i++)
        AWM_HIP_CHECK (hipEventRecord (lane_done[size_t (half) * n_lanes + i], lanes[i]->stream));
      last_half = half;
    }
  // The staging block is the context's: the next call (or the clip `get` with per-clip keys, which stages its group tables through the
  // same block) may write into it as soon as this one returns -- so the last upload out of it has to be through.  Only the copy is
  // awaited, not the clips' kernels.
  if (last_half >= 0)
    AWM_HIP_CHECK (hipEventSynchronize (ev_up[last_half]));
  for (int i = 1; i < n_lanes; i++)
    {
      AWM_HIP_CHECK (hipEventRecord (lanes[i]->ev_sync, lanes[i]->stream));
      AWM_HIP_CHECK (hipStreamWaitEvent (ctx->stream, lanes[i]->ev_sync, 0));
    }
  return rc;
}

int
awm_get_watermark_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels,
                     size_t max_out, awm_pattern *out)
{
  AWM_ENTER (ctx);
  ResultSet rs;
  if (int rc = get_watermark_device (ctx, { capi_key (key) }, make_wav (pcm_d, n_frames, n_channels), rs))
    return rc;
  for (size_t i = 0; i < rs.patterns.size() && i < max_out; i++)
    fill_pattern (rs.patterns[i], out[i]);
  return int (rs.patterns.size());
}


int
awm_get_watermark_keys_d (awm_ctx *ctx, const uint8_t *keys, int n_keys, const float *pcm_d, size_t n_frames, int n_channels,
                          size_t max_out, awm_pattern *out, int *key_of_pattern)
{
  AWM_ENTER (ctx);
  if (n_keys < 0 || (n_keys && !keys) || (max_out && !out))
    {
      set_error ("awm_get_watermark_keys_d: bad argument");
      return AWM_ERR_ARG;
    }
  const std::vector<Key> list = key_list_from (keys, n_keys);
  ResultSet rs;
  if (int rc = get_watermark_device (ctx, list, make_wav (pcm_d, n_frames, n_channels), rs))
    return rc;
  return fill_patterns_keys (rs, list, max_out, out, key_of_pattern);
}

int
awm_get_watermark_s16_d (awm_ctx *ctx, const uint8_t key[16], const int16_t *pcm_d, size_t n_frames, int n_channels,
                         size_t max_out, awm_pattern *out)
{
  AWM_ENTER (ctx);
  if (int rc = check_stream_s16 ("awm_get_watermark_s16_d", pcm_d, n_frames, n_channels))
    return rc;
  ResultSet rs;
  if (int rc = get_watermark_device (ctx, { capi_key (key) }, make_wav_s16 (pcm_d, n_frames, n_channels), rs))
    return rc;
  for (size_t i = 0; i < rs.patterns.size() && i < max_out; i++)
    fill_pattern (rs.patterns[i], out[i]);
  return int (rs.patterns.size());
}

int
awm_get_watermark_keys_s16_d (awm_ctx *ctx, const uint8_t *keys, int n_keys, const int16_t *pcm_d, size_t n_frames, int n_channels,
                              size_t max_out, awm_pattern *out, int *key_of_pattern)
{
  AWM_ENTER (ctx);
  if (n_keys < 0 || (n_keys && !keys) || (max_out && !out))
    {
      set_error ("awm_get_watermark_keys_s16_d: bad argument");
      return AWM_ERR_ARG;
    }
  if (int rc = check_stream_s16 ("awm_get_watermark_keys_s16_d", pcm_d, n_frames, n_channels))
    return rc;
  const std::vector<Key> list = key_list_from (keys, n_keys);
  ResultSet rs;
  if (int rc = get_watermark_device (ctx, list, make_wav_s16 (pcm_d, n_frames, n_channels), rs))
    return rc;
  return fill_patterns_keys (rs, list, max_out, out, key_of_pattern);
}

/* The tail of every batch entry point: the key list -- `key` for all clips, or (keys set) one key per clip --, the batch and its patterns.
 * rates (may be null): the clips are at other rates than 44.1 kHz */
static int
get_batch_tail (awm_ctx *ctx, const uint8_t key[16], const uint8_t *keys, const std::vector<DeviceWav>& clips, const ClipRates *rates, int n_threads,
                size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  if (clips.empty())
    return 0;
  std::vector<Key> clip_keys;
  if (keys)
    clip_keys = key_list_from (keys, int (clips.size()));
  std::vector<ResultSet> sets;
  if (int rc = get_watermark_batch_device (ctx, keys ? std::vector<Key> {} : std::vector<Key> { capi_key (key) }, clips, sets, n_threads,
                                           keys ? &clip_keys : nullptr, rates))
    return rc;
  fill_batch_patterns (sets, max_out_per_clip, out, n_out);
  return 0;
}

/* the clips of a call, clip i at sample_rates[i] (null: every clip at 44.1 kHz); pcm_d null: 16-bit clips, whose values the caller fills in */
static std::vector<DeviceWav>
make_clips (size_t n_clips, const float *const *pcm_d, const size_t *n_frames, int n_channels, const int *sample_rates)
{
  std::vector<DeviceWav> clips;
  for (size_t i = 0; i < n_clips; i++)
    clips.push_back (make_wav_rate (pcm_d ? pcm_d[i] : nullptr, n_frames[i], n_channels, sample_rates ? sample_rates[i] : int (Params::mark_sample_rate)));
  return clips;
}

int
awm_get_watermark_batch_d (awm_ctx *ctx, const uint8_t key[16], size_t n_clips, const float *const *pcm_d, const size_t *n_frames,
                           int n_channels, int n_threads, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  AWM_ENTER (ctx);
  if (n_clips && (!pcm_d || !n_frames || !n_out || (max_out_per_clip && !out)))
    {
      set_error ("awm_get_watermark_batch_d: bad argument");
      return AWM_ERR_ARG;
    }
  return get_batch_tail (ctx, key, nullptr, make_clips (n_clips, pcm_d, n_frames, n_channels, nullptr), nullptr, n_threads, max_out_per_clip, out, n_out);
}

int
awm_get_watermark_batch_keys_d (awm_ctx *ctx, const uint8_t *keys, size_t n_clips, const float *const *pcm_d, const size_t *n_frames,
                                int n_channels, int n_threads, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  AWM_ENTER (ctx);
  if (n_clips && (!keys || !pcm_d || !n_frames || !n_out || (max_out_per_clip && !out)))
    {
      set_error ("awm_get_watermark_batch_keys_d: bad argument");
      return AWM_ERR_ARG;
    }
  return get_batch_tail (ctx, nullptr, keys, make_clips (n_clips, pcm_d, n_frames, n_channels, nullptr), nullptr, n_threads, max_out_per_clip, out, n_out);
}

/* A clip's way through a batch with a rate per clip and its length at 44.1 kHz, without a context (awm_get_batch_rates_plan): false for a
 * rate that is not positive or that neither resampler class takes */
enum { RATES_PATH_GROUP = 0, RATES_PATH_LANE_FIXED = 1, RATES_PATH_LANE_VAR = 2, RATES_PATH_EMPTY = 3 };
static bool
clip_rate_plan (size_t n_frames, int sample_rate, int& path, size_t& n44)
{
  path = -1;
  n44 = 0;
  if (sample_rate <= 0)
    return false;
  bool fixed = true;
  if (sample_rate == Params::mark_sample_rate)
    n44 = n_frames;
  else
    {
      ResampleTable t;
      fixed = resample_fixed_ratio (sample_rate, Params::mark_sample_rate, t.hl, t.np, t.step);
      if (fixed)
        n44 = resample_fixed_frames (t, n_frames);
      else
        {
          const VarResampleGeometry var = var_resample_geometry (double (Params::mark_sample_rate) / sample_rate);
          if (!var.ok)
            return false;
          n44 = var.stream_frames (n_frames);
        }
    }
  path = !n44 ? RATES_PATH_EMPTY : !fixed ? RATES_PATH_LANE_VAR : clip_is_short (n44) ? RATES_PATH_GROUP : RATES_PATH_LANE_FIXED;
  return true;
}

/* the refusals of a call with a rate per clip: AWM_ERR_ARG and a message that names the first offending clip, before anything is enqueued */
static int
check_clip_rates (const char *who, size_t n_clips, const size_t *n_frames, const int *sample_rates)
{
  if (!sample_rates)
    {
      set_error (string_printf ("%s: sample_rates is null", who));
      return AWM_ERR_ARG;
    }
  for (size_t i = 0; i < n_clips; i++)
    {
      int path;
      size_t n44;
      if (!clip_rate_plan (n_frames[i], sample_rates[i], path, n44))
        {
          set_error (string_printf ("%s: clip %zu: resampling from old_rate=%d to new_rate=%d not implemented", who, i, sample_rates[i],
                                    int (Params::mark_sample_rate)));
          return AWM_ERR_ARG;
        }
    }
  return 0;
}

/* `get` at other sample rates: the converters of a call's rates, one table per distinct rate from the context, and every clip's length at
 * 44.1 kHz.  A call at ONE rate hands in n_clips equal rates.  AWM_ERR_ARG (message set) for a rate that awm_resample_frames answers with 0
 * -- the calls with a rate per clip have refused it before (check_clip_rates), naming the clip */
static int
clip_rates_each (awm_ctx *ctx, const int *sample_rates, size_t n_clips, const size_t *n_frames, ClipRates& rates)
{
  std::map<int, RateConverter> convs;
  rates.sample_rate.assign (sample_rates, sample_rates + n_clips);
  rates.table.assign (n_clips, nullptr);
  rates.n44.assign (n_clips, 0);
  for (size_t i = 0; i < n_clips; i++)
    {
      if (sample_rates[i] == Params::mark_sample_rate)
        {
          rates.n44[i] = n_frames[i];
          continue;
        }
      auto it = convs.find (sample_rates[i]);
      if (it == convs.end())
        it = convs.emplace (sample_rates[i], rate_converter (ctx, sample_rates[i], Params::mark_sample_rate)).first;
      if (!it->second.ok())
        {
          set_error (string_printf ("resampling from old_rate=%d to new_rate=%d not implemented", sample_rates[i], int (Params::mark_sample_rate)));
          return AWM_ERR_ARG;
        }
      rates.table[i] = it->second.fixed;
      rates.n44[i] = it->second.stream_frames (n_frames[i]);
    }
  return 0;
}

static bool
rates_all_equal (size_t n_clips, const int *sample_rates)
{
  if (!n_clips || !sample_rates)
    return false;
  for (size_t i = 1; i < n_clips; i++)
    if (sample_rates[i] != sample_rates[0])
      return false;
  return true;
}

/* the batch at ONE other rate (44.1 kHz went to the plain call) */
static int
get_watermark_batch_rate (awm_ctx *ctx, const uint8_t key[16], const uint8_t *keys, size_t n_clips, const float *const *pcm_d, const size_t *n_frames,
                          int n_channels, int sample_rate, int n_threads, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  // (a call without clips is still refused a rate that no resampler takes: one clip of no frames stands in)
  const size_t none = 0;
  const std::vector<int> each (std::max<size_t> (n_clips, 1), sample_rate);
  ClipRates rates;
  if (int rc = clip_rates_each (ctx, each.data(), each.size(), n_clips ? n_frames : &none, rates))
    return rc;
  return get_batch_tail (ctx, key, keys, make_clips (n_clips, pcm_d, n_frames, n_channels, each.data()), &rates, n_threads, max_out_per_clip, out, n_out);
}

int
awm_get_watermark_rate_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels,
                          int sample_rate, size_t max_out, awm_pattern *out)
{
  if (sample_rate == Params::mark_sample_rate)
    return awm_get_watermark_d (ctx, key, pcm_d, n_frames, n_channels, max_out, out);
  AWM_ENTER (ctx);
  if ((n_frames && !pcm_d) || n_channels < 1 || (max_out && !out))
    {
      set_error ("awm_get_watermark_rate_d: bad argument");
      return AWM_ERR_ARG;
    }
  ClipRates rates;
  if (int rc = clip_rates_each (ctx, &sample_rate, 1, &n_frames, rates))
    return rc;
  DeviceWav wav44;
  if (int rc = resample_to_mark_rate (ctx, ctx, rates, 0, make_wav_rate (pcm_d, n_frames, n_channels, sample_rate), wav44))
    return rc;
  ResultSet rs;
  if (int rc = get_watermark_device (ctx, { capi_key (key) }, wav44, rs))
    return rc;
  for (size_t i = 0; i < rs.patterns.size() && i < max_out; i++)
    fill_pattern (rs.patterns[i], out[i]);
  return int (rs.patterns.size());
}

int
awm_get_watermark_rate_s16_d (awm_ctx *ctx, const uint8_t key[16], const int16_t *pcm_d, size_t n_frames, int n_channels,
                              int sample_rate, size_t max_out, awm_pattern *out)
{
  if (sample_rate == Params::mark_sample_rate)
    return awm_get_watermark_s16_d (ctx, key, pcm_d, n_frames, n_channels, max_out, out);
  AWM_ENTER (ctx);
  if (max_out && !out)
    {
      set_error ("awm_get_watermark_rate_s16_d: bad argument");
      return AWM_ERR_ARG;
    }
  if (int rc = check_stream_s16 ("awm_get_watermark_rate_s16_d", pcm_d, n_frames, n_channels))
    return rc;
  ClipRates rates;
  if (int rc = clip_rates_each (ctx, &sample_rate, 1, &n_frames, rates))
    return rc;
  // (the 44.1 kHz copy on the lane is float: from here on the call is the float call's)
  DeviceWav wav44;
  if (int rc = resample_to_mark_rate (ctx, ctx, rates, 0, make_wav_s16 (pcm_d, n_frames, n_channels, sample_rate), wav44))
    return rc;
  ResultSet rs;
  if (int rc = get_watermark_device (ctx, { capi_key (key) }, wav44, rs))
    return rc;
  for (size_t i = 0; i < rs.patterns.size() && i < max_out; i++)
    fill_pattern (rs.patterns[i], out[i]);
  return int (rs.patterns.size());
}

int
awm_get_watermark_batch_rate_d (awm_ctx *ctx, const uint8_t key[16], size_t n_clips, const float *const *pcm_d, const size_t *n_frames,
                                int n_channels, int sample_rate, int n_threads, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  if (sample_rate == Params::mark_sample_rate)
    return awm_get_watermark_batch_d (ctx, key, n_clips, pcm_d, n_frames, n_channels, n_threads, max_out_per_clip, out, n_out);
  AWM_ENTER (ctx);
  if (n_clips && (!pcm_d || !n_frames || !n_out || (max_out_per_clip && !out)))
    {
      set_error ("awm_get_watermark_batch_rate_d: bad argument");
      return AWM_ERR_ARG;
    }
  return get_watermark_batch_rate (ctx, key, nullptr, n_clips, pcm_d, n_frames, n_channels, sample_rate, n_threads, max_out_per_clip, out, n_out);
}

int
awm_get_watermark_batch_keys_rate_d (awm_ctx *ctx, const uint8_t *keys, size_t n_clips, const float *const *pcm_d, const size_t *n_frames,
                                     int n_channels, int sample_rate, int n_threads, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  if (sample_rate == Params::mark_sample_rate)
    return awm_get_watermark_batch_keys_d (ctx, keys, n_clips, pcm_d, n_frames, n_channels, n_threads, max_out_per_clip, out, n_out);
  AWM_ENTER (ctx);
  if (n_clips && (!keys || !pcm_d || !n_frames || !n_out || (max_out_per_clip && !out)))
    {
      set_error ("awm_get_watermark_batch_keys_rate_d: bad argument");
      return AWM_ERR_ARG;
    }
  return get_watermark_batch_rate (ctx, nullptr, keys, n_clips, pcm_d, n_frames, n_channels, sample_rate, n_threads, max_out_per_clip, out, n_out);
}

int
awm_debug_clip_stage_d (awm_ctx *ctx, size_t n_clips, const float *const *pcm_d, const size_t *n_frames, int n_channels, int sample_rate,
                        float *slices_d, long long *range_out)
{
  AWM_ENTER (ctx);
  if (!n_clips || !pcm_d || !n_frames || n_channels < 1)
    {
      set_error ("awm_debug_clip_stage_d: bad argument");
      return AWM_ERR_ARG;
    }
  const std::vector<int> each (n_clips, sample_rate);
  ClipRates rates;
  const bool at_rate = sample_rate != Params::mark_sample_rate;
  if (at_rate)
    if (int rc = clip_rates_each (ctx, each.data(), n_clips, n_frames, rates))
      return rc;
  return clip_stage_device (ctx, make_clips (n_clips, pcm_d, n_frames, n_channels, each.data()), at_rate ? &rates : nullptr, slices_d, range_out);
}

/* the refusals, the converters and the float clips of a call with a rate per clip */
static int
clips_rates (awm_ctx *ctx, const char *who, size_t n_clips, const float *const *pcm_d, const size_t *n_frames, int n_channels, const int *sample_rates,
             ClipRates& rates, std::vector<DeviceWav>& clips)
{
  if (int rc = check_clip_rates (who, n_clips, n_frames, sample_rates))
    return rc;
  if (int rc = clip_rates_each (ctx, sample_rates, n_clips, n_frames, rates))
    return rc;
  clips = make_clips (n_clips, pcm_d, n_frames, n_channels, sample_rates);
  return 0;
}

/* The batches on 16-bit clips (awm_get_watermark_batch_rates_s16_d and its twins): the refusals, the converters and the clips of a call.
 * sample_rates may be null (every clip at 44.1 kHz).  Always the path with a rate per clip: a group that shares one rate runs the one-rate
 * stage there as well, and a call at 44.1 kHz the copy */
static int
clips_s16 (awm_ctx *ctx, const char *who, size_t n_clips, const int16_t *const *pcm_d, const size_t *n_frames, int n_channels, const int *sample_rates,
           ClipRates& rates, std::vector<DeviceWav>& clips)
{
  std::vector<int> mark_rates;
  if (!sample_rates)
    {
      mark_rates.assign (n_clips, int (Params::mark_sample_rate));
      sample_rates = mark_rates.data();
    }
  if (int rc = check_clip_rates (who, n_clips, n_frames, sample_rates))
    return rc;
  for (size_t i = 0; i < n_clips; i++)
    if ((reinterpret_cast<uintptr_t> (pcm_d[i]) & 1) || (!pcm_d[i] && n_frames[i]))
      {
        set_error (string_printf ("%s: clip %zu: %s", who, i, pcm_d[i] ? "pcm_d is not 2-byte aligned" : "pcm_d is null"));
        return AWM_ERR_ARG;
      }
  if (int rc = clip_rates_each (ctx, sample_rates, n_clips, n_frames, rates))
    return rc;
  clips = make_clips (n_clips, nullptr, n_frames, n_channels, sample_rates);
  for (size_t i = 0; i < n_clips; i++)
    clips[i].pcm16 = pcm_d[i];
  return 0;
}

/* the batch with a rate per clip, float (pcm_d) or 16-bit (pcm16_d) clips, after the entry point's own checks */
static int
get_watermark_batch_each (awm_ctx *ctx, const char *who, const uint8_t key[16], const uint8_t *keys, size_t n_clips, const float *const *pcm_d,
                          const int16_t *const *pcm16_d, const size_t *n_frames, int n_channels, const int *sample_rates, int n_threads,
                          size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  if (!n_clips)
    return 0;
  if ((!pcm_d && !pcm16_d) || !n_frames || !n_out || (max_out_per_clip && !out) || (!key && !keys) || n_channels < 1)
    {
      set_error (string_printf ("%s: bad argument", who));
      return AWM_ERR_ARG;
    }
  ClipRates rates;
  std::vector<DeviceWav> clips;
  if (int rc = pcm16_d ? clips_s16 (ctx, who, n_clips, pcm16_d, n_frames, n_channels, sample_rates, rates, clips)
                       : clips_rates (ctx, who, n_clips, pcm_d, n_frames, n_channels, sample_rates, rates, clips))
    return rc;
  return get_batch_tail (ctx, key, keys, clips, &rates, n_threads, max_out_per_clip, out, n_out);
}

int
awm_get_watermark_batch_rates_d (awm_ctx *ctx, const uint8_t key[16], size_t n_clips, const float *const *pcm_d, const size_t *n_frames,
                                 int n_channels, const int *sample_rates, int n_threads, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  if (rates_all_equal (n_clips, sample_rates))           // IS the one-rate function (which hands 44.1 kHz on), before anything else happens
    return awm_get_watermark_batch_rate_d (ctx, key, n_clips, pcm_d, n_frames, n_channels, sample_rates[0], n_threads, max_out_per_clip, out, n_out);
  AWM_ENTER (ctx);
  if (n_clips && !key)
    {
      set_error ("awm_get_watermark_batch_rates_d: bad argument");
      return AWM_ERR_ARG;
    }
  return get_watermark_batch_each (ctx, "awm_get_watermark_batch_rates_d", key, nullptr, n_clips, pcm_d, nullptr, n_frames, n_channels, sample_rates,
                                   n_threads, max_out_per_clip, out, n_out);
}

int
awm_get_watermark_batch_keys_rates_d (awm_ctx *ctx, const uint8_t *keys, size_t n_clips, const float *const *pcm_d, const size_t *n_frames,
                                      int n_channels, const int *sample_rates, int n_threads, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  if (rates_all_equal (n_clips, sample_rates))
    return awm_get_watermark_batch_keys_rate_d (ctx, keys, n_clips, pcm_d, n_frames, n_channels, sample_rates[0], n_threads, max_out_per_clip, out,
                                                n_out);
  AWM_ENTER (ctx);
  if (n_clips && !keys)
    {
      set_error ("awm_get_watermark_batch_keys_rates_d: bad argument");
      return AWM_ERR_ARG;
    }
  return get_watermark_batch_each (ctx, "awm_get_watermark_batch_keys_rates_d", nullptr, keys, n_clips, pcm_d, nullptr, n_frames, n_channels,
                                   sample_rates, n_threads, max_out_per_clip, out, n_out);
}

int
awm_debug_clip_stage_rates_d (awm_ctx *ctx, size_t n_clips, const float *const *pcm_d, const size_t *n_frames, int n_channels, const int *sample_rates,
                              float *slices_d, long long *range_out)
{
  AWM_ENTER (ctx);
  if (!n_clips || !pcm_d || !n_frames || n_channels < 1)
    {
      set_error ("awm_debug_clip_stage_rates_d: bad argument");
      return AWM_ERR_ARG;
    }
  ClipRates rates;
  std::vector<DeviceWav> clips;
  if (int rc = clips_rates (ctx, "awm_debug_clip_stage_rates_d", n_clips, pcm_d, n_frames, n_channels, sample_rates, rates, clips))
    return rc;
  return clip_stage_device (ctx, clips, &rates, slices_d, range_out);
}

int
awm_get_watermark_batch_rates_s16_d (awm_ctx *ctx, const uint8_t key[16], size_t n_clips, const int16_t *const *pcm_d, const size_t *n_frames,
                                     int n_channels, const int *sample_rates, int n_threads, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  AWM_ENTER (ctx);
  return get_watermark_batch_each (ctx, "awm_get_watermark_batch_rates_s16_d", key, nullptr, n_clips, nullptr, pcm_d, n_frames, n_channels, sample_rates,
                                   n_threads, max_out_per_clip, out, n_out);
}

int
awm_get_watermark_batch_keys_rates_s16_d (awm_ctx *ctx, const uint8_t *keys, size_t n_clips, const int16_t *const *pcm_d, const size_t *n_frames,
                                          int n_channels, const int *sample_rates, int n_threads, size_t max_out_per_clip, awm_pattern *out, int *n_out)
{
  AWM_ENTER (ctx);
  return get_watermark_batch_each (ctx, "awm_get_watermark_batch_keys_rates_s16_d", nullptr, keys, n_clips, nullptr, pcm_d, n_frames, n_channels,
                                   sample_rates, n_threads, max_out_per_clip, out, n_out);
}

int
awm_debug_clip_stage_rates_s16_d (awm_ctx *ctx, size_t n_clips, const int16_t *const *pcm_d, const size_t *n_frames, int n_channels,
                                  const int *sample_rates, float *slices_d, long long *range_out)
{
  AWM_ENTER (ctx);
  if (!n_clips || !pcm_d || !n_frames || n_channels < 1)
    {
      set_error ("awm_debug_clip_stage_rates_s16_d: bad argument");
      return AWM_ERR_ARG;
    }
  ClipRates rates;
  std::vector<DeviceWav> clips;
  if (int rc = clips_s16 (ctx, "awm_debug_clip_stage_rates_s16_d", n_clips, pcm_d, n_frames, n_channels, sample_rates, rates, clips))
    return rc;
  return clip_stage_device (ctx, clips, &rates, slices_d, range_out);
}

int
awm_get_batch_rates_plan (size_t n_clips, const size_t *n_frames, const int *sample_rates, int *path_out, size_t *n44_out)
{
  if (n_clips && (!n_frames || !sample_rates))
    {
      set_error ("awm_get_batch_rates_plan: bad argument");
      return AWM_ERR_ARG;
    }
  int rc = 0;
  for (size_t i = 0; i < n_clips; i++)
    {
      int path;
      size_t n44;
      if (!clip_rate_plan (n_frames[i], sample_rates[i], path, n44) && !rc)
        {
          set_error (string_printf ("awm_get_batch_rates_plan: clip %zu: resampling from old_rate=%d to new_rate=%d not implemented", i, sample_rates[i],
                                    int (Params::mark_sample_rate)));
          rc = AWM_ERR_ARG;
        }
      if (path_out)
        path_out[i] = path;
      if (n44_out)
        n44_out[i] = n44;
    }
  return rc;
}

int
awm_decode_chunks_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels,
                     int n_chunks, const uint64_t *first_frame, const uint64_t *chunk_frames, int first_is_stream_start,
                     size_t max_out, awm_pattern *out, int *chunk_of_pattern)
{
  AWM_ENTER (ctx);
  std::vector<ChunkRange> chunks;
  for (int i = 0; i < n_chunks; i++)
    {
      if (first_frame[i] + chunk_frames[i] > n_frames)
        {
          set_error ("awm_decode_chunks_d: chunk exceeds the buffer");
          return AWM_ERR_ARG;
        }
      chunks.push_back ({ size_t (first_frame[i]), size_t (chunk_frames[i]), 0.0 });
    }
  std::vector<ResultSet> sets;
  if (int rc = decode_chunks (ctx, { capi_key (key) }, make_wav (pcm_d, n_frames, n_channels), chunks, first_is_stream_start != 0, sets))
    return rc;
  size_t n = 0;
  for (size_t c = 0; c < sets.size(); c++)
    {
      auto& pats = sets[c].patterns;
      std::stable_sort (pats.begin(), pats.end(), [] (const ResultSet::Pattern& a, const ResultSet::Pattern& b) { return a.time < b.time; });
      for (const auto& p : pats)
        {
          if (n < max_out)
            {
              fill_pattern (p, out[n]);
              chunk_of_pattern[n] = int (c);
            }
          n++;
        }
    }
  return int (n);
}

/* ---- file level: the reference's add_watermark / get_watermark (wmcommon.hh:226-228) ------------------------------------ */
namespace {
// --input-format raw / --output-format raw with the --raw-* options for the duration of one call (the reference keeps
// these in the process-global Params, wmcommon.hh:79-83)
struct FormatScope
{
  Format old_in = params().input_format, old_out = params().output_format;
  RawFormat old_raw_in = StreamParams::raw_input_format, old_raw_out = StreamParams::raw_output_format;
  static bool
  apply (const awm_raw_format *f, Format& format, RawFormat& raw)
  {
    if (!f)
      {
        format = Format::AUTO;
        return true;
      }
    if (f->n_channels < 1 || f->sample_rate < 1 || !pcm_format_ok (f->bit_depth, f->encoding))
      return false;
    format = Format::RAW;
    raw.n_channels = f->n_channels;
    raw.sample_rate = f->sample_rate;
    raw.bit_depth = f->bit_depth;
    raw.encoding = f->encoding == 0 ? Encoding::SIGNED : f->encoding == 1 ? Encoding::UNSIGNED : Encoding::FLOAT;
    raw.endian = f->big_endian ? RawFormat::BIG : RawFormat::LITTLE;
    return true;
  }
  ~FormatScope()
  {
    params().input_format = old_in;
    params().output_format = old_out;
    StreamParams::raw_input_format = old_raw_in;
    StreamParams::raw_output_format = old_raw_out;
  }
};
}

int
awm_add_watermark_file (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const char *in_path, const char *out_path,
                        const awm_raw_format *raw_in, const awm_raw_format *raw_out)
{
  AWM_ENTER (ctx);
  if (!payload_hex || !in_path || !out_path)
    {
      set_error ("awm_add_watermark_file: bad argument");
      return AWM_ERR_ARG;
    }
  FormatScope scope;
  if (!FormatScope::apply (raw_in, params().input_format, StreamParams::raw_input_format)
      || !FormatScope::apply (raw_out, params().output_format, StreamParams::raw_output_format))
    {
      set_error ("awm_add_watermark_file: unsupported raw format");
      return AWM_ERR_ARG;
    }
  file_fail_reset();
  return add_watermark (ctx, capi_key (key), in_path, out_path, payload_hex) ? file_fail_kind() : 0;
}

int
awm_add_stream_watermark_file (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const char *in_path, const char *out_path,
                               const awm_raw_format *raw_in, const awm_raw_format *raw_out, size_t zero_frames)
{
  AWM_ENTER (ctx);
  if (!payload_hex || !in_path || !out_path)
    {
      set_error ("awm_add_stream_watermark_file: bad argument");
      return AWM_ERR_ARG;
    }
  FormatScope scope;
  if (!FormatScope::apply (raw_in, params().input_format, StreamParams::raw_input_format)
      || !FormatScope::apply (raw_out, params().output_format, StreamParams::raw_output_format))
    {
      set_error ("awm_add_stream_watermark_file: unsupported raw format");
      return AWM_ERR_ARG;
    }
  file_fail_reset();
  return add_watermark_at (ctx, capi_key (key), in_path, out_path, payload_hex, zero_frames) ? file_fail_kind() : 0;
}

/* two paths that name the same file: equal strings, or both exist and are one inode */
static bool
same_file (const char *a, const char *b)
{
  if (!std::strcmp (a, b))
    return true;
  struct stat sa, sb;
  return stat (a, &sa) == 0 && stat (b, &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

int
awm_add_stream_watermark_payloads_file (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads,
                                        const char *in_path, const char *const *out_path,
                                        const awm_raw_format *raw_in, const awm_raw_format *raw_out, size_t zero_frames)
{
  AWM_ENTER (ctx);
  if (!n_payloads)
    return 0;
  if (!key || !payload_hex || !in_path || !out_path)
    {
      set_error ("awm_add_watermark_payloads_file: bad argument");
      return AWM_ERR_ARG;
    }
  // everything is checked before a file is opened: creating an output truncates what is there
  std::vector<std::string> outfiles, bits;
  for (size_t p = 0; p < n_payloads; p++)
    {
      if (!payload_hex[p] || !out_path[p])
        {
          set_error (string_printf ("awm_add_watermark_payloads_file: null pointer at index %zu", p));
          return AWM_ERR_ARG;
        }
      if (parse_payload (payload_hex[p]).empty())
        {
          set_error (string_printf ("awm_add_watermark_payloads_file: cannot parse payload '%s' at index %zu", payload_hex[p], p));
          return AWM_ERR_ARG;
        }
      if (same_file (out_path[p], in_path))
        {
          set_error (string_printf ("awm_add_watermark_payloads_file: output path %zu is the input path", p));
          return AWM_ERR_ARG;
        }
      for (size_t q = 0; q < p; q++)
        if (same_file (out_path[p], out_path[q]))
          {
            set_error (string_printf ("awm_add_watermark_payloads_file: output paths %zu and %zu are equal", q, p));
            return AWM_ERR_ARG;
          }
      outfiles.push_back (out_path[p]);
      bits.push_back (payload_hex[p]);
    }
  FormatScope scope;
  if (!FormatScope::apply (raw_in, params().input_format, StreamParams::raw_input_format)
      || !FormatScope::apply (raw_out, params().output_format, StreamParams::raw_output_format))
    {
      set_error ("awm_add_watermark_payloads_file: unsupported raw format");
      return AWM_ERR_ARG;
    }
  file_fail_reset();
  return add_watermark_payloads_at (ctx, capi_key (key), in_path, outfiles, bits, zero_frames) ? file_fail_kind() : 0;
}

int
awm_add_watermark_payloads_file (awm_ctx *ctx, const uint8_t key[16], const char *const *payload_hex, size_t n_payloads,
                                 const char *in_path, const char *const *out_path,
                                 const awm_raw_format *raw_in, const awm_raw_format *raw_out)
{
  return awm_add_stream_watermark_payloads_file (ctx, key, payload_hex, n_payloads, in_path, out_path, raw_in, raw_out, 0);
}

int
awm_add_get_watermark_file (awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const char *in_path, const char *out_path,
                            const awm_raw_format *raw_in, const awm_raw_format *raw_out, size_t max_out, awm_pattern *out)
{
  AWM_ENTER (ctx);
  if (!payload_hex || !in_path || !out_path || (max_out && !out))
    {
      set_error ("awm_add_get_watermark_file: bad argument");
      return AWM_ERR_ARG;
    }
  FormatScope scope;
  if (!FormatScope::apply (raw_in, params().input_format, StreamParams::raw_input_format)
      || !FormatScope::apply (raw_out, params().output_format, StreamParams::raw_output_format))
    {
      set_error ("awm_add_get_watermark_file: unsupported raw format");
      return AWM_ERR_ARG;
    }
  ResultSet rs;
  file_fail_reset();
  if (add_get_watermark (ctx, capi_key (key), in_path, out_path, payload_hex, rs))
    return file_fail_kind();
  for (size_t i = 0; i < rs.patterns.size() && i < max_out; i++)
    fill_pattern (rs.patterns[i], out[i]);
  return int (rs.patterns.size());
}

int
awm_get_watermark_file (awm_ctx *ctx, const uint8_t key[16], const char *in_path, const awm_raw_format *raw_in,
                        size_t max_out, awm_pattern *out)
{
  AWM_ENTER (ctx);
  if (!in_path || (max_out && !out))
    {
      set_error ("awm_get_watermark_file: bad argument");
      return AWM_ERR_ARG;
    }
  FormatScope scope;
  if (!FormatScope::apply (raw_in, params().input_format, StreamParams::raw_input_format))
    {
      set_error ("awm_get_watermark_file: unsupported raw format");
      return AWM_ERR_ARG;
    }
  Error err;
  auto in_stream = AudioInputStream::create (in_path, err);
  if (err)
    {
      set_error (std::string ("error loading ") + in_path + ": " + err.message());
      return AWM_ERR_IO;
    }
  ResultSet rs;
  size_t n_values = 0;
  file_fail_reset();
  if (get_watermark_stream (ctx, { capi_key (key) }, in_stream.get(), false, rs, n_values, in_path))
    return file_fail_kind();
  for (size_t i = 0; i < rs.patterns.size() && i < max_out; i++)
    fill_pattern (rs.patterns[i], out[i]);
  return int (rs.patterns.size());
}

int
awm_get_watermark_keys_file (awm_ctx *ctx, const uint8_t *keys, int n_keys, const char *in_path, const awm_raw_format *raw_in,
                             size_t max_out, awm_pattern *out, int *key_of_pattern)
{
  AWM_ENTER (ctx);
  if (!in_path || n_keys < 0 || (n_keys && !keys) || (max_out && !out))
    {
      set_error ("awm_get_watermark_keys_file: bad argument");
      return AWM_ERR_ARG;
    }
  FormatScope scope;
  if (!FormatScope::apply (raw_in, params().input_format, StreamParams::raw_input_format))
    {
      set_error ("awm_get_watermark_keys_file: unsupported raw format");
      return AWM_ERR_ARG;
    }
  Error err;
  auto in_stream = AudioInputStream::create (in_path, err);
  if (err)
    {
      set_error (std::string ("error loading ") + in_path + ": " + err.message());
      return AWM_ERR_IO;
    }
  const std::vector<Key> list = key_list_from (keys, n_keys);
  ResultSet rs;
  size_t n_values = 0;
  file_fail_reset();
  if (get_watermark_stream (ctx, list, in_stream.get(), false, rs, n_values, in_path))
    return file_fail_kind();
  return fill_patterns_keys (rs, list, max_out, out, key_of_pattern);
}

int
awm_plan_chunks (size_t n_frames, size_t max_out, uint64_t *first_frame, uint64_t *chunk_frames, double *time_offset)
{
  const auto chunks = plan_chunks (n_frames, 1);
  for (size_t i = 0; i < chunks.size() && i < max_out; i++)
    {
      first_frame[i] = chunks[i].first_frame;
      chunk_frames[i] = chunks[i].n_frames;
      time_offset[i] = chunks[i].time_offset;
    }
  return int (chunks.size());
}

int
awm_merge_patterns (const uint8_t key[16], const awm_pattern *patterns, const int *chunk_count, int n_chunks,
                    size_t max_out, awm_pattern *out)
{
  const Key k = capi_key (key);
  ResultSet result;
  size_t pos = 0;
  for (int c = 0; c < n_chunks; c++)
    {
      ResultSet chunk;
      for (int i = 0; i < chunk_count[c]; i++, pos++)
        {
          const awm_pattern& p = patterns[pos];
          SyncFinder::Score score { size_t (p.sync_index), p.sync_quality, ConvBlockType (p.block_type) };
          chunk.add_pattern (k, p.time, score, std::vector<int> (p.bits, p.bits + p.n_bits), p.decode_error,
                             ResultSet::Type (p.type), p.speed);
        }
      result.merge (chunk);
    }
  result.sort ({ k });
  for (size_t i = 0; i < result.patterns.size() && i < max_out; i++)
    fill_pattern (result.patterns[i], out[i]);
  return int (result.patterns.size());
}

int
awm_decode_chunk_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels,
                    int first_chunk, size_t max_out, awm_pattern *out)
{
  AWM_ENTER (ctx);
  ResultSet rs;
  if (int rc = decode_chunk (ctx, rs, { capi_key (key) }, make_wav (pcm_d, n_frames, n_channels), first_chunk != 0))
    return rc;
  std::stable_sort (rs.patterns.begin(), rs.patterns.end(), [] (const ResultSet::Pattern& a, const ResultSet::Pattern& b) { return a.time < b.time; });
  for (size_t i = 0; i < rs.patterns.size() && i < max_out; i++)
    fill_pattern (rs.patterns[i], out[i]);
  return int (rs.patterns.size());
}

/* ---- speed detection (reference wmspeed.cc) ---------------------------------------------------------------------- */
void
awm_set_speed_params (int detect_speed, int detect_speed_patient, double try_speed, double test_speed)
{
  ParamValues& g = global_params();
  g.detect_speed = detect_speed != 0;
  g.detect_speed_patient = detect_speed_patient != 0;
  g.try_speed = try_speed;
  g.test_speed = test_speed;
}

size_t
awm_resample_ratio_frames (size_t n_frames, int n_channels, int rate, double ratio, double max_in_seconds)
{
  size_t in_frames = n_frames;
  if (max_in_seconds > 0)
    in_frames = std::min<size_t> (in_frames * n_channels, n_channels * lrint (rate * max_in_seconds)) / n_channels;
  return size_t (lrint (in_frames * ratio));
}

int
awm_resample_ratio_d (awm_ctx *ctx, const float *pcm_in_d, size_t n_frames, int n_channels, int rate, double ratio,
                      double max_in_seconds, float *out_d, size_t n_out_frames)
{
  AWM_ENTER (ctx);
  if ((n_frames && !pcm_in_d) || (n_out_frames && !out_d) || n_channels < 1 || rate < 1)
    {
      set_error ("awm_resample_ratio_d: bad argument");
      return AWM_ERR_ARG;
    }
  DevBuffer tmp;
  size_t n_out = 0;
  int rc = resample_ratio_device (ctx, ctx, make_wav_rate (pcm_in_d, n_frames, n_channels, rate), ratio, max_in_seconds, tmp, &n_out);
  if (!rc)
    {
      const size_t n = std::min (n_out, n_out_frames) * n_channels * sizeof (float);
      if (n && hipMemcpyAsync (out_d, tmp.ptr, n, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
        rc = AWM_ERR_HIP;
      if (!rc && hipStreamSynchronize (ctx->stream) != hipSuccess)
        rc = AWM_ERR_HIP;
    }
  tmp.release();
  return rc;
}

int
awm_speed_clip_location_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int rate,
                           double seconds, int candidates, double *location)
{
  AWM_ENTER (ctx);
  return speed_clip_location (ctx, ctx, capi_key (key), make_wav_rate (pcm_d, n_frames, n_channels, rate), seconds, candidates, location);
}

int
awm_speed_mags_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int rate,
                  double clip_location, double center, double seconds, size_t max_rows, float *out)
{
  AWM_ENTER (ctx);
  std::vector<float> m;
  int rows = 0;
  if (int rc = speed_mags (ctx, ctx, capi_key (key), make_wav_rate (pcm_d, n_frames, n_channels, rate), clip_location, center, seconds, m, &rows))
    return rc;
  std::copy (m.begin(), m.begin() + std::min<size_t> (rows, max_rows) * 510 * 2, out);
  return rows;
}

namespace {
// the scores of a pass as the scan entry points give them out: sorted by speed, up to max_out of them
void
write_scores_by_speed (std::vector<SpeedScore>& scores, size_t max_out, double *out_speed, double *out_quality)
{
  std::sort (scores.begin(), scores.end(), [] (const SpeedScore& a, const SpeedScore& b) { return a.speed < b.speed; });
  for (size_t i = 0; i < scores.size() && i < max_out; i++)
    {
      out_speed[i] = scores[i].speed;
      out_quality[i] = scores[i].quality;
    }
}
}

int
awm_speed_scan_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int rate,
                  double clip_location, double seconds, double step, int n_steps, int n_center_steps,
                  const double *speeds, int n_speeds, size_t max_out, double *out_speed, double *out_quality)
{
  AWM_ENTER (ctx);
  std::vector<SpeedScore> scores;
  if (int rc = speed_scan (ctx, ctx, capi_key (key), make_wav_rate (pcm_d, n_frames, n_channels, rate), clip_location,
                           { seconds, step, n_steps, n_center_steps }, std::vector<double> (speeds, speeds + n_speeds), scores))
    return rc;
  write_scores_by_speed (scores, max_out, out_speed, out_quality);
  return int (scores.size());
}

int
awm_detect_speed_d (awm_ctx *ctx, const uint8_t key[16], const float *pcm_d, size_t n_frames, int n_channels, int rate,
                    int patient, double *speed_out, double *quality_out)
{
  AWM_ENTER (ctx);
  const bool old_patient = params().detect_speed_patient;
  params().detect_speed_patient = patient != 0;
  std::vector<DetectSpeedResult> results;
  double speed = 0, quality = 0;
  const int rc = detect_speed (ctx, ctx, { capi_key (key) }, make_wav_rate (pcm_d, n_frames, n_channels, rate), nullptr, results, &speed, &quality);
  params().detect_speed_patient = old_patient;
  if (rc)
    return rc;
  if (speed_out)
    *speed_out = speed;
  if (quality_out)
    *quality_out = quality;
  return results.empty() ? 0 : 1;
}

/* ---- batches of clips ---- */
namespace {
// the checks the batch entry points share: AWM_ERR_ARG before anything is enqueued or written
int
speed_batch_args (const char *what, const uint8_t *keys, size_t n_clips, const float *const *pcm_d, const size_t *n_frames, int n_channels, int rate)
{
  bool bad = n_channels < 1 || rate <= 0 || (n_clips && (!keys || !pcm_d || !n_frames));
  for (size_t i = 0; i < n_clips && !bad; i++)
    bad = !pcm_d[i] && n_frames[i] > 0;
  if (bad)
    {
      set_error (std::string (what) + ": bad argument");
      return AWM_ERR_ARG;
    }
  return 0;
}
}

void
awm_debug_set_speed_batch_bytes (size_t bytes)
{
  speed_batch_set_bytes (bytes);
}

size_t
awm_debug_speed_batch_bytes (void)
{
  return speed_batch_bytes();
}

int
awm_speed_batch_plan (size_t n_clips, const size_t *n_frames, int n_channels, int rate, int patient, size_t budget_bytes, int *group_of_clip,
                      size_t *bytes_of_group)
{
  if (n_channels < 1 || rate <= 0 || (n_clips && (!n_frames || !group_of_clip)))
    {
      set_error ("awm_speed_batch_plan: bad argument");
      return AWM_ERR_ARG;
    }
  std::vector<int> group;
  std::vector<size_t> bytes;
  const int n = speed_batch_plan (std::vector<size_t> (n_frames, n_frames + n_clips), std::vector<int> (n_clips, rate), n_channels, patient != 0,
                                  budget_bytes ? budget_bytes : speed_batch_bytes(), group, bytes);
  std::copy (group.begin(), group.end(), group_of_clip);
  if (bytes_of_group)
    std::copy (bytes.begin(), bytes.end(), bytes_of_group);
  return n;
}

int
awm_detect_speed_batch_d (awm_ctx *ctx, const uint8_t *keys, int key_per_clip, size_t n_clips, const float *const *pcm_d, const size_t *n_frames,
                          int n_channels, int rate, int patient, double *speed_out, double *quality_out, int *use_out)
{
  AWM_ENTER (ctx);
  if (int rc = speed_batch_args ("awm_detect_speed_batch_d", keys, n_clips, pcm_d, n_frames, n_channels, rate))
    return rc;
  if (!n_clips)
    return 0;
  std::vector<SpeedBatchClip> clips;
  for (size_t i = 0; i < n_clips; i++)
    clips.push_back ({ capi_key (keys + (key_per_clip ? 16 * i : 0)), make_wav_rate (pcm_d[i], n_frames[i], n_channels, rate) });
  const bool old_patient = params().detect_speed_patient;
  params().detect_speed_patient = patient != 0;
  std::vector<SpeedBatchResult> results;
  const int rc = detect_speed_batch (ctx, ctx, clips, results);
  params().detect_speed_patient = old_patient;
  if (rc)
    return rc;
  for (size_t i = 0; i < n_clips; i++)
    {
      if (speed_out)
        speed_out[i] = results[i].speed;
      if (quality_out)
        quality_out[i] = results[i].quality;
      if (use_out)
        use_out[i] = results[i].rc ? results[i].rc : results[i].use ? 1 : 0;
    }
  return 0;
}

int
awm_debug_speed_scan_batch_d (awm_ctx *ctx, const uint8_t *keys, int key_per_clip, size_t n_clips, const float *const *pcm_d, const size_t *n_frames,
                              int n_channels, int rate, const double *clip_locations, double seconds, double step, int n_steps, int n_center_steps,
                              const double *speeds, const int *n_speeds, size_t max_out_per_clip, double *out_speed, double *out_quality, int *n_out)
{
  AWM_ENTER (ctx);
  if (int rc = speed_batch_args ("awm_debug_speed_scan_batch_d", keys, n_clips, pcm_d, n_frames, n_channels, rate))
    return rc;
  if (n_clips && (!clip_locations || !speeds || !n_speeds || !n_out || (max_out_per_clip && (!out_speed || !out_quality))))
    {
      set_error ("awm_debug_speed_scan_batch_d: bad argument");
      return AWM_ERR_ARG;
    }
  std::vector<SpeedBatchItem> items (n_clips);
  std::vector<SpeedBatchItem *> batch;
  size_t at = 0;
  for (size_t i = 0; i < n_clips; i++)
    {
      items[i].key = capi_key (keys + (key_per_clip ? 16 * i : 0));
      items[i].wav = make_wav_rate (pcm_d[i], n_frames[i], n_channels, rate);
      items[i].clip_location = clip_locations[i];
      items[i].speeds.assign (speeds + at, speeds + at + std::max (n_speeds[i], 0));
      at += std::max (n_speeds[i], 0);
      batch.push_back (&items[i]);
    }
  if (int rc = speed_scan_batch (ctx, ctx, batch, { seconds, step, n_steps, n_center_steps }))
    return rc;
  for (size_t i = 0; i < n_clips; i++)
    {
      write_scores_by_speed (items[i].scores, max_out_per_clip, out_speed + i * max_out_per_clip, out_quality + i * max_out_per_clip);
      n_out[i] = items[i].rc ? items[i].rc : int (items[i].scores.size());
    }
  return 0;
}

} // extern "C"
