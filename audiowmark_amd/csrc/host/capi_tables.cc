// C ABI: key-derived tables (pure host; usable without a GPU) -- see include/awm_hip.h
#include "context.hh"
#include "utils.hh"
#include "wmspeed.hh"
#include "random.hh"
#include <algorithm>
#include <cstring>
#include <memory>

using namespace awm;

static Key
key_from_bytes (const uint8_t key[16])
{
  Key k;
  k.set_raw (key);
  return k;
}

namespace awm { Key capi_key (const uint8_t key[16]) { return key_from_bytes (key); } }

extern "C" {

int
awm_tab_up_down (const uint8_t key[16], int stream, int frame, int up[30], int down[30])
{
  UpDownGen gen (key_from_bytes (key), Random::Stream (stream));
  UpDownArray u, d;
  gen.get (frame, u, d);
  for (int i = 0; i < 30; i++)
    {
      up[i] = u[i];
      down[i] = d[i];
    }
  return 0;
}

int
awm_test_gen_noise (const uint8_t key[16], size_t n_values, float *out)
{
  // reference audiowmark.cc:399-417 (test-gen-noise): uniform [-1, 1) from the data_up_down stream, seed 0
  Random rng (key_from_bytes (key), 0, Random::Stream::data_up_down);
  for (size_t i = 0; i < n_values; i++)
    out[i] = float (rng.random_double() * 2 - 1);
  return 0;
}

int
awm_tab_bit_pos (const uint8_t key[16], int pos[AWM_BLOCK_FRAMES])
{
  BitPosGen gen (key_from_bytes (key));
  const int ns = mark_sync_frame_count(), nd = mark_data_frame_count();
  for (int f = 0; f < ns; f++)
    pos[f] = gen.sync_frame (f);
  for (int f = 0; f < nd; f++)
    pos[ns + f] = gen.data_frame (f);
  return ns + nd;
}

int
awm_tab_mix_entries (const uint8_t key[16], int *out)
{
  const auto entries = gen_mix_entries (key_from_bytes (key));
  for (size_t i = 0; i < entries.size(); i++)
    {
      out[3 * i] = entries[i].frame;
      out[3 * i + 1] = entries[i].up;
      out[3 * i + 2] = entries[i].down;
    }
  return int (entries.size());
}

int
awm_tab_bit_order (const uint8_t key[16], size_t n, unsigned *order)
{
  const auto o = bit_order (key_from_bytes (key), n);
  std::copy (o.begin(), o.end(), order);
  return 0;
}

int
awm_tab_frame_mod (const uint8_t key[16], const char *payload_hex, int8_t *out)
{
  const auto bits = parse_payload (payload_hex ? payload_hex : "");
  if (bits.empty())
    {
      set_error ("cannot parse payload");
      return AWM_ERR_ARG;
    }
  const auto table = build_frame_mod_table (key_from_bytes (key), bits);
  std::memcpy (out, table.data(), table.size());
  return int (table.size());
}

int
awm_tab_frame_mod_template (const uint8_t key[16], int16_t *out)
{
  if (!key)
    {
      set_error ("awm_tab_frame_mod_template: bad argument");
      return AWM_ERR_ARG;
    }
  if (!out)                                                // (the size alone: 2 * mark_block_frame_count() * n_bands entries)
    return int (2 * mark_block_frame_count() * Params::n_bands);
  const auto table = build_frame_mod_template (key_from_bytes (key));
  std::memcpy (out, table.data(), table.size() * sizeof (int16_t));
  return int (table.size());
}

int
awm_tab_sync_bits (const uint8_t key[16], int clip_mode, int *out)
{
  const auto t = build_sync_table (key_from_bytes (key), clip_mode != 0);
  size_t o = 0;
  for (size_t r = 0; r < t.frame.size(); r++)
    {
      out[o++] = t.frame[r];
      for (int i = 0; i < 30; i++) out[o++] = t.up[r * 30 + i];
      for (int i = 0; i < 30; i++) out[o++] = t.down[r * 30 + i];
    }
  return t.rows_per_bit;
}

int
awm_tab_window (size_t n, float *out)
{
  const auto w = gen_normalized_window (n);
  std::copy (w.begin(), w.end(), out);
  return 0;
}

int
awm_tab_synth_window (float *out)
{
  const auto w = gen_synth_window();
  std::copy (w.begin(), w.end(), out);
  return 0;
}

/* The window of one stream segment at another sample rate (include/awm_hip.h).  With b_X (m) = floor (m step_X /
 * np_X), output m of resampler X reads inputs b_X (m) - hl_X + 1 ... b_X (m) + hl_X of its stream (kernels.hh ResampleArgs), so the
 * smallest m that reaches input j is ceil ((j - hl_X) np_X / step_X).  Every index is below 2^40 + 2^12 at the stream's rate and below
 * 2^45 at 44.1 kHz (the down ratio is at least 1 / 16), np <= 1000 and step <= 16000 (Resampler::setup): every product below fits 2^59. */
int
awm_add_segment_plan (int sample_rate, size_t zero_frames, size_t n_frames, awm_segment_plan *plan)
{
  if (!plan)
    {
      set_error ("awm_add_segment_plan: bad argument");
      return AWM_ERR_ARG;
    }
  *plan = awm_segment_plan {};
  int hd, nd, sd, hu, nu, su;
  if (sample_rate <= 0 || !resample_fixed_ratio (sample_rate, Params::mark_sample_rate, hd, nd, sd)
      || !resample_fixed_ratio (Params::mark_sample_rate, sample_rate, hu, nu, su))
    {
      set_error (string_printf ("awm_add_segment_plan: no fixed-ratio resampler between %d Hz and %d Hz", sample_rate, Params::mark_sample_rate));
      return AWM_ERR_ARG;
    }
  constexpr uint64_t LIMIT = uint64_t (1) << 40;
  if (uint64_t (zero_frames) >= LIMIT || uint64_t (n_frames) >= LIMIT || uint64_t (zero_frames) + uint64_t (n_frames) >= LIMIT)
    {
      set_error ("awm_add_segment_plan: zero_frames + n_frames must stay below 2^40");
      return AWM_ERR_ARG;
    }
  plan->down_hl = hd; plan->down_np = nd; plan->down_step = sd;
  plan->up_hl = hu; plan->up_np = nu; plan->up_step = su;
  plan->limiter_block = uint64_t (sample_rate) * uint64_t (Params::limiter_block_size_ms) / 1000;
  if (!n_frames || !plan->limiter_block)
    return 0;
  const uint64_t FRAME = Params::frame_size, Z = zero_frames, n = n_frames;
  auto b = [] (uint64_t m, int step, int np) { return m * uint64_t (step) / uint64_t (np); };
  auto first_reaching = [] (uint64_t j, int hl, int step, int np) {            // the smallest m with b (m) + hl >= j
    return j <= uint64_t (hl) ? uint64_t (0) : ((j - uint64_t (hl)) * uint64_t (np) + uint64_t (step) - 1) / uint64_t (step);
  };
  // in front of the segment the stream is silent, but the watermark is not: the first 44.1 kHz sample that sees the segment lies in frame
  // f0, whose spectrum also shapes frame f0 - 1; the first output the up-resampler makes from those frames is where the mix begins
  const uint64_t f0 = first_reaching (Z, hd, sd, nd) / FRAME;
  const uint64_t w0 = (f0 ? f0 - 1 : 0) * FRAME;
  plan->mix_first = std::min<uint64_t> (Z, first_reaching (w0, hu, su, nu));
  // up: watermark samples the outputs mix_first ... Z + n - 1 read, and their frames
  const uint64_t ub = b (plan->mix_first, su, nu), wm_first = ub + 1 > uint64_t (hu) ? ub + 1 - uint64_t (hu) : 0;
  const uint64_t wm_last = b (Z + n - 1, su, nu) + uint64_t (hu);
  plan->frame_first = wm_first / FRAME;
  plan->frame_last = wm_last / FRAME;
  // K2: a frame is complete once both neighbours were transformed (frame 0 has none in front)
  plan->slice_first = plan->frame_first ? plan->frame_first - 1 : 0;
  plan->slice_last = plan->frame_last + 1;
  // down: the samples of those frames, and the part of the segment they read
  plan->down_first = plan->slice_first * FRAME;
  plan->down_last = (plan->slice_last + 1) * FRAME - 1;
  const uint64_t db = b (plan->down_first, sd, nd), in_lo = db + 1 > uint64_t (hd) ? db + 1 - uint64_t (hd) : 0;
  const uint64_t in_hi = b (plan->down_last, sd, nd) + uint64_t (hd);
  plan->in_first = in_lo > Z ? std::min (in_lo - Z, n - 1) : 0;
  plan->in_last = in_hi >= Z ? std::min (in_hi - Z, n - 1) : 0;
  plan->first_block = plan->mix_first / plan->limiter_block;
  plan->n_blocks = (Z + n) / plan->limiter_block + 2 - plan->first_block;
  return 0;
}

/* The look-ahead of the tile stream at another sample rate (include/awm_hip.h), with awm_add_segment_plan's window
 * rule.  The mix of output m reads watermark samples up to wl = b_up (m) + hl_up, which lie in frame f = wl / 1024; that frame is complete
 * once frame f + 1 was transformed, whose last sample q = (f + 2) 1024 - 1 reads the stream up to b_down (q) + hl_down.  For one f the
 * distance to m is largest at the first m that reaches the frame, and the whole chain repeats after lcm (1024, np_down) samples at 44.1 kHz
 * (np_down / gcd (np_down, 1024) <= 1000 frames): one loop over those frames finds the maximum. */
int
awm_add_stream_rate_plan (int sample_rate, awm_stream_rate_plan *plan)
{
  if (!plan)
    {
      set_error ("awm_add_stream_rate_plan: bad argument");
      return AWM_ERR_ARG;
    }
  *plan = awm_stream_rate_plan {};
  awm_segment_plan tables;
  if (awm_add_segment_plan (sample_rate, 0, 0, &tables) || !tables.limiter_block)
    {
      set_error (string_printf ("awm_add_stream_rate_plan: no fixed-ratio resampler between %d Hz and %d Hz", sample_rate,
                                Params::mark_sample_rate));
      return AWM_ERR_ARG;
    }
  const int hd = tables.down_hl, nd = tables.down_np, sd = tables.down_step, hu = tables.up_hl, nu = tables.up_np, su = tables.up_step;
  plan->down_hl = hd; plan->down_np = nd; plan->down_step = sd;
  plan->up_hl = hu; plan->up_np = nu; plan->up_step = su;
  plan->limiter_block = tables.limiter_block;
  plan->down_ahead = uint64_t (hd);                // 44.1 kHz sample q reads b_down (q) - hl + 1 ... b_down (q) + hl
  const uint64_t FRAME = Params::frame_size;
  uint64_t period = uint64_t (nd), two = FRAME;    // frames after which the chain repeats: np_down / gcd (np_down, 1024)
  while (two > 1 && period % 2 == 0)
    {
      period /= 2;
      two /= 2;
    }
  uint64_t ahead = 0;
  for (uint64_t f = 0; f <= period + 1; f++)
    {
      const uint64_t j = f * FRAME;                // the first m with b_up (m) + hl_up >= j
      const uint64_t m = j <= uint64_t (hu) ? 0 : ((j - uint64_t (hu)) * uint64_t (nu) + uint64_t (su) - 1) / uint64_t (su);
      const uint64_t q = (f + 2) * FRAME - 1;
      const uint64_t last_in = q * uint64_t (sd) / uint64_t (nd) + uint64_t (hd);
      if (last_in > m)
        ahead = std::max (ahead, last_in - m);
    }
  plan->mix_ahead = ahead;
  /* Tile t is limited once the block behind its last sample is mixed: up to 2 limiter blocks - 1 behind its end.  After the push of tile
   * t + 2 the mix has reached 2 tiles - mix_ahead - (what the launches that end on multiples of np hold back: less than down_step + up_np + 1
   * <= mix_ahead) behind that end, so one limiter block + mix_ahead per tile is enough; and never less than the 44.1 kHz object's 128 frames. */
  const uint64_t need = plan->limiter_block + plan->mix_ahead;
  plan->min_tile = std::max<uint64_t> (128 * FRAME, (need + FRAME - 1) / FRAME * FRAME);
  return 0;
}

int
awm_conv_encode (int block_type, const int *bits, size_t n, int *out)
{
  if (block_type < 0 || block_type > 2)
    return AWM_ERR_ARG;
  const auto r = conv_encode (ConvBlockType (block_type), std::vector<int> (bits, bits + n));
  std::copy (r.begin(), r.end(), out);
  return int (r.size());
}

/* ---- host side pieces of the speed detection (no GPU needed) ---------------------------------------------------- */
int
awm_speed_select_n_best (double *speed, double *quality, int count, int n)
{
  std::vector<SpeedScore> scores (count);
  for (int i = 0; i < count; i++)
    {
      scores[i].speed = speed[i];
      scores[i].quality = quality[i];
    }
  select_n_best_scores (scores, size_t (n));
  for (size_t i = 0; i < scores.size(); i++)
    {
      speed[i] = scores[i].speed;
      quality[i] = scores[i].quality;
    }
  return int (scores.size());
}

double
awm_speed_smooth_best (const double *speed, const double *quality, int count, double step, double distance)
{
  std::vector<SpeedScore> scores (count);
  for (int i = 0; i < count; i++)
    {
      scores[i].speed = speed[i];
      scores[i].quality = quality[i];
    }
  return count ? score_smooth_find_best (scores, step, distance) : 0;
}

size_t
awm_speed_clip_positions (const uint8_t key[16], size_t n_values, size_t max_out, uint64_t *positions)
{
  Random rng (key_from_bytes (key), 0, Random::Stream::speed_clip);
  size_t count = 0;
  for (size_t p = 0; p < n_values; p += rng() % 1000)
    {
      if (count < max_out)
        positions[count] = p;
      count++;
    }
  return count;
}

int
awm_speed_clip_candidates (const uint8_t key[16], const float *hashed_values, size_t n, int candidates, double *locations)
{
  unsigned char hash[20];
  sha1 (hashed_values, n * sizeof (float), hash);
  uint64_t seed = 0;
  for (int i = 0; i < 8; i++)
    seed = (seed << 8) | hash[i];
  Random rng (key_from_bytes (key), seed, Random::Stream::speed_clip);
  for (int c = 0; c < candidates; c++)
    locations[c] = rng.random_double();
  return 0;
}

int
awm_var_resample_table (double ratio, float *out, size_t max_floats, int *hl_out)
{
  int hl = 0;
  const std::vector<float> tab = var_resample_table (ratio, &hl);
  if (tab.empty())
    {
      set_error (string_printf ("failed to setup vresampler with ratio=%f", ratio));
      return AWM_ERR_ARG;
    }
  if (hl_out)
    *hl_out = hl;
  if (out)
    std::copy (tab.begin(), tab.begin() + std::min (tab.size(), max_floats), out);
  return int (tab.size());
}

void
awm_set_params (double water_delta, int mix, int frames_per_bit, int test_no_limiter,
                double sync_threshold2, int n_best, double chunk_size_min)
{
  ParamValues& g = global_params();
  g.water_delta = water_delta;
  g.mix = mix != 0;
  g.frames_per_bit = frames_per_bit;
  g.test_no_limiter = test_no_limiter != 0;
  g.sync_threshold2 = sync_threshold2;
  g.get_n_best = n_best;
  g.get_chunk_size = chunk_size_min;
}

/* ---- the whole parameter set, process-wide or per context (awm_hip.h: awm_params) ---- */
static void
params_to_c (const ParamValues& v, awm_params *p)
{
  p->struct_size = sizeof (awm_params);
  p->water_delta = v.water_delta;
  p->mix = v.mix;
  p->hard = v.hard;
  p->strict = v.strict;
  p->snr = v.snr;
  p->payload_size = int (v.payload_size);
  p->frames_per_bit = v.frames_per_bit;
  p->sync_threshold2 = v.sync_threshold2;
  p->get_n_best = v.get_n_best;
  p->get_chunk_size = v.get_chunk_size;
  p->detect_speed = v.detect_speed;
  p->detect_speed_patient = v.detect_speed_patient;
  p->try_speed = v.try_speed;
  p->test_speed = v.test_speed;
  p->test_cut = v.test_cut;
  p->test_no_sync = v.test_no_sync;
  p->test_no_limiter = v.test_no_limiter;
  p->test_truncate = v.test_truncate;
}

static int
params_from_c (const awm_params *p, ParamValues& v)
{
  if (!p || p->struct_size != sizeof (awm_params))
    {
      set_error ("awm_params: struct_size does not match this library (use awm_params_init)");
      return AWM_ERR_ARG;
    }
  if (!(p->water_delta >= 0) || p->payload_size < 1 || p->frames_per_bit < 1 || p->get_n_best < 1 || !(p->get_chunk_size > 0))
    {
      set_error ("awm_params: value out of range");
      return AWM_ERR_ARG;
    }
  v.water_delta = p->water_delta;
  v.mix = p->mix != 0;
  v.hard = p->hard != 0;
  v.strict = p->strict != 0;
  v.snr = p->snr != 0;
  v.payload_size = size_t (p->payload_size);
  v.frames_per_bit = p->frames_per_bit;
  v.sync_threshold2 = p->sync_threshold2;
  v.get_n_best = p->get_n_best;
  v.get_chunk_size = p->get_chunk_size;
  v.detect_speed = p->detect_speed != 0;
  v.detect_speed_patient = p->detect_speed_patient != 0;
  v.try_speed = p->try_speed;
  v.test_speed = p->test_speed;
  v.test_cut = p->test_cut;
  v.test_no_sync = p->test_no_sync != 0;
  v.test_no_limiter = p->test_no_limiter != 0;
  v.test_truncate = p->test_truncate;
  return 0;
}

void
awm_params_init (awm_params *p)
{
  if (p)
    params_to_c (ParamValues(), p);
}

int
awm_set_global_params (const awm_params *p)
{
  ParamValues v = global_params();          // (what awm_params does not carry -- formats, json output -- stays)
  if (int rc = params_from_c (p, v))
    return rc;
  global_params() = v;
  return 0;
}

int
awm_ctx_set_params (awm_ctx *ctx, const awm_params *p)
{
  if (!ctx)
    {
      set_error ("null context");
      return AWM_ERR_ARG;
    }
  if (!p)
    {
      ctx->own_params.reset();
      return 0;
    }
  auto v = std::make_unique<ParamValues> (ctx->own_params ? *ctx->own_params : global_params());
  if (int rc = params_from_c (p, *v))
    return rc;
  ctx->own_params = std::move (v);
  return 0;
}

int
awm_ctx_get_params (const awm_ctx *ctx, awm_params *out)
{
  if (!out)
    return AWM_ERR_ARG;
  params_to_c (ctx && ctx->own_params ? *ctx->own_params : global_params(), out);
  return 0;
}

/* -q / --quiet of the command line (reference audiowmark.cc:1020-1023): information messages off */
void
awm_set_quiet (int quiet)
{
  set_log_level (quiet ? Log::WARNING : Log::INFO);
}

} // extern "C"
