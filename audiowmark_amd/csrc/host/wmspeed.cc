// wmspeed.cc -- speed detection (reference src/wmspeed.cc) driven from the host, computed on the GPU (hip/speed.hip).
#include "wmspeed.hh"
#include "wmcommon.hh"
#include "utils.hh"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <thread>

namespace awm {

void
SpeedWorkspace::release()
{
  for (auto& sl : table_slabs)
    sl.buf.release();
  table_slabs.clear();
  var_tables.clear();
  for (auto& t : key_tables)
    {
      t->cols.release();
      t->col_frame.release();
      t->col_first.release();
    }
  window512.release();
}

void
SpeedScratch::release()
{
  for (DevBuffer *b : { &sub, &mags, &centers, &best, &gather_pos, &gather_out, &ranges, &energy, &stretched })
    b->release();
  pin.release();
}

SpeedScratch *
speed_scratch (WorkLane *lane)
{
  if (!lane->speed_scratch)
    lane->speed_scratch = new SpeedScratch();
  return lane->speed_scratch;
}

void
speed_scratch_free (WorkLane *lane)
{
  if (lane->speed_scratch)
    {
      lane->speed_scratch->release();
      delete lane->speed_scratch;
      lane->speed_scratch = nullptr;
    }
}

void
speed_workspace_free (awm_ctx *ctx)
{
  if (ctx->speed)
    {
      ctx->speed->release();
      delete ctx->speed;
      ctx->speed = nullptr;
    }
}

namespace {

SpeedWorkspace *
workspace (awm_ctx *ctx)
{
  if (!ctx->speed)
    ctx->speed = new SpeedWorkspace();
  return ctx->speed;
}

/* zita VResampler::setup (ratio, nchan, hlen = 16) geometry: taps per side, relative cutoff, phase step 256 / ratio */
struct VarGeometry
{
  bool     ok = false;
  unsigned hl = 0;
  double   frel = 0, step = 0;
};
VarGeometry
var_geometry (double ratio)
{
  VarGeometry g;
  const unsigned hlen = 16;
  if (!(16 * ratio >= 1) || ratio > 256)
    return g;
  g.frel = 1.0 - 2.6 / hlen;
  g.step = 256 / ratio;
  g.hl = hlen;
  if (ratio < 1)
    {
      g.frel *= ratio;
      g.hl = unsigned (std::ceil (hlen / ratio));
    }
  g.ok = true;
  return g;
}

/* tables for all ratios of a pass (the missing ones are computed on a few host threads: 257 x hl sinc / window values each) */
int
get_var_tables (awm_ctx *ctx, const std::vector<double>& ratios, std::vector<VarResampleTable *>& out)
{
  std::lock_guard<std::mutex> lock (ctx->speed_mutex);        // the table caches are shared by the lanes
  SpeedWorkspace *ws = workspace (ctx);
  out.assign (ratios.size(), nullptr);
  std::vector<size_t> missing;
  for (size_t i = 0; i < ratios.size(); i++)
    {
      for (auto& t : ws->var_tables)
        if (t->ratio == ratios[i])
          out[i] = t.get();
      for (size_t j = 0; j < i && !out[i]; j++)
        if (ratios[j] == ratios[i])
          out[i] = out[j];                               // filled in below through the first occurrence
      if (!out[i] && std::find_if (missing.begin(), missing.end(), [&] (size_t m) { return ratios[m] == ratios[i]; }) == missing.end())
        missing.push_back (i);
    }
  std::vector<std::vector<float>> tabs (missing.size());
  std::vector<VarGeometry> geo (missing.size());
  for (size_t k = 0; k < missing.size(); k++)
    {
      geo[k] = var_geometry (ratios[missing[k]]);
      if (!geo[k].ok)
        {
          set_error (string_printf ("failed to setup vresampler with ratio=%f", ratios[missing[k]]));
          return AWM_ERR_ARG;
        }
    }
  const size_t n_threads = std::min<size_t> (missing.size(), std::max (1u, std::min (16u, std::thread::hardware_concurrency())));
  std::vector<std::thread> threads;
  for (size_t t = 0; t < n_threads; t++)
    threads.emplace_back ([&, t] {
      for (size_t k = t; k < missing.size(); k += n_threads)
        {
          // rows padded to an odd stride (the kernel keeps the table in LDS: equal columns of different rows -> different banks)
          const std::vector<float> dense = zita_table (geo[k].frel, geo[k].hl, 256);
          const size_t hl = geo[k].hl, stride = hl | 1;
          tabs[k].assign (257 * stride, 0.f);
          for (size_t r = 0; r < 257; r++)
            std::copy (dense.begin() + r * hl, dense.begin() + (r + 1) * hl, tabs[k].begin() + r * stride);
        }
    });
  for (auto& th : threads)
    th.join();
  if (!missing.empty())
    {
      // one device allocation and one copy for all tables this call adds (every table 16 byte aligned inside the slab)
      std::vector<size_t> at (missing.size());
      size_t total = 0;
      for (size_t k = 0; k < missing.size(); k++)
        {
          at[k] = total;
          total += (tabs[k].size() + 3) & ~size_t (3);
        }
      std::vector<float> blob (total, 0.f);
      for (size_t k = 0; k < missing.size(); k++)
        std::copy (tabs[k].begin(), tabs[k].end(), blob.begin() + at[k]);
      VarTableSlab slab;
      slab.serial = ws->next_slab++;
      if (int rc = upload_sync (slab.buf, blob.data(), blob.size() * sizeof (float), ctx->stream))
        return rc;
      for (size_t k = 0; k < missing.size(); k++)
        {
          auto vt = std::make_unique<VarResampleTable>();
          vt->ratio = ratios[missing[k]];
          vt->hl = int (geo[k].hl);
          vt->ctab = slab.buf.as<float>() + at[k];
          vt->slab = slab.serial;
          ws->var_tables.push_back (std::move (vt));
        }
      ws->table_slabs.push_back (slab);
      // Bounded cache.  The grids of the first pass (57 centres each for the normal and the patient search) never change and are in
      // the first slabs ever made: those stay; beyond max_tables the OLDEST of the data dependent refinement slabs goes, with all
      // its tables.  (Nothing handed out by this call is dropped: a call either finds all its ratios, or adds the missing ones
      // last.  Up to CHUNK_LANES searches run side by side, each with ~100 ratios of its own in use: the cache is an order of
      // magnitude larger than that, so the oldest slab is never one a running search holds.  A table is ~20 KB.)
      constexpr size_t keep_slabs = 2, max_tables = 4096;
      while (ws->var_tables.size() > max_tables && ws->table_slabs.size() > keep_slabs + 1)
        {
          const size_t gone = ws->table_slabs[keep_slabs].serial;
          ws->table_slabs[keep_slabs].buf.release();
          ws->table_slabs.erase (ws->table_slabs.begin() + keep_slabs);
          ws->var_tables.erase (std::remove_if (ws->var_tables.begin(), ws->var_tables.end(),
                                                [&] (const std::unique_ptr<VarResampleTable>& t) { return t->slab == gone; }),
                                ws->var_tables.end());
        }
    }
  for (size_t i = 0; i < ratios.size(); i++)
    if (!out[i])
      for (auto& t : ws->var_tables)
        if (t->ratio == ratios[i])
          out[i] = t.get();
  return 0;
}

/* device description of one resampler run */
awmk::SpeedCenterDev
center_dev (const VarResampleTable *vt, double ratio, long long n_in, long long n_out)
{
  awmk::SpeedCenterDev cd {};
  const VarResampleGeometry g = var_resample_geometry (ratio);     // (ok: the ratio has a table)
  cd.ctab = vt->ctab;
  cd.hl = vt->hl;
  cd.stride = vt->hl | 1;
  cd.mant = g.mant;
  cd.shift = g.shift;
  cd.frac_scale = std::ldexp (1.0, 8 - g.shift);           // step = mant * 2^(e - 53), e - 53 = 8 - shift
  cd.n_in = n_in;
  cd.n_out = n_out;
  cd.rows = 0;
  return cd;
}

SpeedKeyTables *
get_speed_key_tables (awm_ctx *ctx, const Key& key)
{
  std::lock_guard<std::mutex> lock (ctx->speed_mutex);
  SpeedWorkspace *ws = workspace (ctx);
  std::vector<unsigned char> kb (key.aes_key(), key.aes_key() + Key::SIZE);
  for (auto& t : ws->key_tables)
    if (t->key == kb && t->frames_per_bit == params().frames_per_bit)
      return t.get();
  KeyTables *kt = ctx->get_key_tables (key);
  if (!kt)
    return nullptr;
  const SyncTable& st = kt->sync[0].host;                  // BLOCK mode: 6 x 85 rows sorted by frame within a bit
  const int R = st.rows_per_bit;
  std::vector<unsigned int> cols (size_t (6) * R * 16, 0);
  std::vector<int> col_frame (size_t (6) * R);
  for (int col = 0; col < 6 * R; col++)
    {
      unsigned char *bytes = reinterpret_cast<unsigned char *> (&cols[size_t (col) * 16]);
      for (int i = 0; i < 30; i++)
        {
          bytes[i] = st.up[size_t (col) * 30 + i];
          bytes[30 + i] = st.down[size_t (col) * 30 + i];
        }
      col_frame[col] = st.frame[col];
    }
  const int fpb = int (mark_block_frame_count());
  std::vector<unsigned char> col_first (size_t (6) * (fpb + 2), 0);
  for (int bit = 0; bit < 6; bit++)
    for (int f = 0; f < fpb + 2; f++)
      {
        int count = 0;
        for (int r = 0; r < R; r++)
          count += st.frame[size_t (bit) * R + r] < f;
        col_first[size_t (bit) * (fpb + 2) + f] = (unsigned char) count;
      }
  auto t = std::make_unique<SpeedKeyTables>();
  t->key = kb;
  t->frames_per_bit = params().frames_per_bit;
  if (upload_sync (t->col_first, col_first.data(), col_first.size(), ctx->stream))
    return nullptr;
  if (upload_sync (t->cols, cols.data(), cols.size() * sizeof (unsigned int), ctx->stream))
    return nullptr;
  if (upload_sync (t->col_frame, col_frame.data(), col_frame.size() * sizeof (int), ctx->stream))
    return nullptr;
  ws->key_tables.push_back (std::move (t));
  return ws->key_tables.back().get();
}

int
ensure_window (awm_ctx *ctx)
{
  std::lock_guard<std::mutex> lock (ctx->speed_mutex);
  SpeedWorkspace *ws = workspace (ctx);
  if (ws->window512.ptr)
    return 0;
  const std::vector<float> win = gen_normalized_window (Params::frame_size / 2);
  return upload_sync (ws->window512, win.data(), win.size() * sizeof (float), ctx->stream);
}

/* get_speed_clip (reference wmspeed.cc:33-52): frame range of the clip */
void
speed_clip_range (double location, const DeviceWav& wav, double clip_seconds, size_t *start_point, size_t *end_point)
{
  const double end_sec = double (wav.n_frames) / wav.sample_rate;
  double start_sec = location * (end_sec - clip_seconds);
  if (start_sec < 0)
    start_sec = 0;
  *start_point = start_sec * wav.sample_rate;
  *end_point = std::min<size_t> (*start_point + clip_seconds * wav.sample_rate, wav.n_frames);
}

struct ScanCenter { double speed; VarResampleTable *table; long long n_in, n_out; int rows; };

/* resample_ratio_truncate (clip, center / 2, mark_sample_rate / 2, seconds / center) and the STFT rows of its output */
void
center_geometry (const DeviceWav& clip, double seconds, ScanCenter& c)
{
  const int C = clip.n_channels, N = Params::frame_size / 2, hop = Params::sync_search_step / 2;
  size_t in_frames = clip.n_frames;
  const double max_in_seconds = seconds / c.speed;
  if (max_in_seconds > 0)
    in_frames = std::min<size_t> (in_frames * C, C * lrint (clip.sample_rate * max_in_seconds)) / C;
  c.n_in = (long long) in_frames;
  c.n_out = lrint (in_frames * (c.speed / 2));             // "we downsample the audio by factor 2 to improve performance"
  c.rows = c.n_out > N ? int ((c.n_out - N - 1) / hop + 1) : 0;          // pos + N < n_out, pos = 0, hop, ...
}

/* the three passes of run_search (reference wmspeed.cc:622-681) */
struct SearchPlan
{
  SpeedScanParams scan1, scan2, scan3;
  size_t n_best;
};
SearchPlan
search_plan (bool patient)
{
  // first pass: grid over 0.8 .. 1.25; second: improve the n best; third: fast refinement around the best
  SearchPlan p;
  p.scan1 = patient ? SpeedScanParams { 50, 1.00035, 11, 28 } : SpeedScanParams { 25, 1.0007, 5, 28 };
  p.scan2 = patient ? SpeedScanParams { 50, 1.000175, 1, 0 } : SpeedScanParams { 50, 1.00035, 1, 0 };
  p.scan3 = SpeedScanParams { 50, 1.00005, 40, 0 };
  p.n_best = patient ? 15 : 5;
  return p;
}
constexpr double scan3_smooth_distance = 20;
constexpr double speed_sync_threshold = 0.4;
constexpr int    clip_candidates = 5;

/* "our algorithm won't work at all for very short input files" */
bool
long_enough_to_search (size_t n_frames, int rate)
{
  return rate > 0 && double (n_frames) / rate >= 0.25;
}

/* the part of the input a pass reads (SpeedSearch::get_jobs, reference wmspeed.cc:461-492): "speed is between 0.8 and 1.25, so we
 * use a clip seconds factor of 1.3 to provide enough samples" */
DeviceWav
scan_clip (const DeviceWav& wav, double clip_location, const SpeedScanParams& sp)
{
  size_t start_point, end_point;
  speed_clip_range (clip_location, wav, sp.seconds * 1.3, &start_point, &end_point);
  DeviceWav clip = wav;
  clip.data = wav.data + start_point * wav.n_channels;
  clip.n_frames = end_point - start_point;
  return clip;
}

/* the centres of a pass around `speed`, -n_center_steps .. n_center_steps */
void
append_centers (const SpeedScanParams& sp, double speed, std::vector<ScanCenter>& centers)
{
  for (int c = -sp.n_center_steps; c <= sp.n_center_steps; c++)
    centers.push_back ({ speed * std::pow (sp.step, c * (sp.n_steps * 2 + 1)), nullptr, 0, 0, 0 });
}

/* sub and mags keep one stride per launch, the largest any of its centres needs (the pass reserves them, the planner counts them) */
struct PassStrides
{
  long long max_out = 0;
  int       max_rows = 0;
  void      add (const ScanCenter& c)    { max_out = std::max (max_out, c.n_out); max_rows = std::max (max_rows, c.rows); }
  void      add (const PassStrides& s)   { max_out = std::max (max_out, s.max_out); max_rows = std::max (max_rows, s.max_rows); }
  long long sub_stride (int C) const     { return (max_out * C + 3) / 4 * 4; }
  long long ld() const                   { return (max_rows + 15) / 16 * 16; }
  long long center_stride() const        { return 510 * ld(); }
};

} // namespace

DevBuffer&
speed_stretch_buffer (WorkLane *lane)
{
  return speed_scratch (lane)->stretched;
}

VarResampleGeometry
var_resample_geometry (double ratio)
{
  VarResampleGeometry g;
  const VarGeometry vg = var_geometry (ratio);
  if (!vg.ok)
    return g;
  int e = 0;
  const double f = std::frexp (vg.step, &e);               // step = f * 2^e, 0.5 <= f < 1
  g.ok = true;
  g.hl = int (vg.hl);
  g.mant = (unsigned long long) std::ldexp (f, 53);        // step = mant * 2^(e - 53)
  g.shift = 61 - e;                                        // m * step / 256 = (m * mant) >> shift
  return g;
}

std::vector<float>
var_resample_table (double ratio, int *hl)
{
  const VarGeometry vg = var_geometry (ratio);
  if (!vg.ok)
    return {};
  *hl = int (vg.hl);
  return zita_table (vg.frel, vg.hl, 256);
}

int
resample_var_device (awm_ctx *ctx, WorkLane *lane, const float *in_d, size_t n_in, int n_channels, double ratio, float *out_d, size_t n_out)
{
  SpeedScratch *ws = speed_scratch (lane);
  std::vector<VarResampleTable *> tables;
  if (int rc = get_var_tables (ctx, { ratio }, tables))
    return rc;
  if (!n_out)
    return 0;
  const awmk::SpeedCenterDev cd = center_dev (tables[0], ratio, (long long) n_in, (long long) n_out);
  if (int rc = ws->centers.reserve (sizeof (cd)))
    return rc;
  hipStream_t st = lane->stream;
  AWM_HIP_CHECK (hipMemcpyAsync (ws->centers.ptr, &cd, sizeof (cd), hipMemcpyHostToDevice, st));
  AWM_HIP_CHECK (hipStreamSynchronize (st));
  awmk::VarResampleArgs ra {};
  ra.in = in_d;
  ra.n_channels = n_channels;
  ra.centers = ws->centers.as<awmk::SpeedCenterDev>();
  ra.out = out_d;
  ra.out_stride = 0;
  ra.max_stride = cd.stride;
  ra.max_step = std::ldexp (double (cd.mant), -cd.shift);
  {
    ProfScope ps (ctx, PROF_RESAMPLE_VAR, double (n_in + n_out) * n_channels * 4.0, st);
    AWM_HIP_CHECK (awmk::launch_resample_var (st, ra, (long long) n_out, 1));
  }
  AWM_HIP_CHECK (hipStreamSynchronize (st));
  return 0;
}

int
resample_ratio_device (awm_ctx *ctx, WorkLane *lane, const DeviceWav& wav, double ratio, double max_in_seconds, DevBuffer& out,
                       size_t *n_out_frames)
{
  const int C = wav.n_channels;
  size_t in_frames = wav.n_frames;
  if (max_in_seconds > 0)
    in_frames = std::min<size_t> (in_frames * C, C * lrint (wav.sample_rate * max_in_seconds)) / C;
  if (!var_geometry (ratio).ok)
    {
      set_error (string_printf ("failed to setup vresampler with ratio=%f", ratio));
      return AWM_ERR_ARG;
    }
  const long long n_out = lrint (in_frames * ratio);
  *n_out_frames = size_t (n_out);
  if (int rc = out.reserve (std::max<size_t> (size_t (n_out) * C * sizeof (float), 16)))
    return rc;
  return resample_var_device (ctx, lane, wav.data, in_frames, C, ratio, out.as<float>(), size_t (n_out));
}

void
select_n_best_scores (std::vector<SpeedScore>& scores, size_t n)
{
  std::sort (scores.begin(), scores.end(), [] (const SpeedScore& a, const SpeedScore& b) { return a.speed < b.speed; });
  const auto quality_at = [&] (int pos) { return pos >= 0 && size_t (pos) < scores.size() ? scores[pos].quality : 0.0; };
  std::vector<SpeedScore> peaks;
  for (int x = 0; size_t (x) < scores.size(); x++)
    {
      // single peak, or the first of two equal values that are larger than their outer neighbours
      if (quality_at (x - 1) <= quality_at (x) && quality_at (x) >= quality_at (x + 1))
        {
          peaks.push_back (scores[x]);
          x++;                                             // its right neighbour cannot be a local maximum
        }
    }
  std::sort (peaks.begin(), peaks.end(), [] (const SpeedScore& a, const SpeedScore& b) { return a.quality > b.quality; });
  if (peaks.size() > n)
    peaks.resize (n);
  scores = peaks;
}

double
score_smooth_find_best (const std::vector<SpeedScore>& in_scores, double step, double distance)
{
  std::vector<SpeedScore> scores = in_scores;
  std::sort (scores.begin(), scores.end(), [] (const SpeedScore& a, const SpeedScore& b) { return a.speed < b.speed; });
  const auto window_cos = [] (double x) { return std::fabs (x) > 1 ? 0.0 : 0.5 * std::cos (x * M_PI) + 0.5; };   // von Hann
  double best_speed = 0, best_quality = 0;
  for (double speed = scores.front().speed; speed < scores.back().speed; speed += 0.000001)
    {
      double quality_sum = 0, quality_div = 0;
      for (const auto& s : scores)
        {
          const double w = window_cos ((s.speed - speed) / (step * distance));
          quality_sum += s.quality * w;
          quality_div += w;
        }
      quality_sum /= quality_div;
      if (quality_sum > best_quality)
        {
          best_speed = speed;
          best_quality = quality_sum;
        }
    }
  return best_speed;
}

/* ------------------------------------------------------------------------------------------------------------------
 * The search: clip location, three passes and the decisions between them, for one clip (SpeedForm::ONE_CLIP) or for
 * several clips in lockstep (SpeedForm::BATCH).  An entry of a launch is a (clip, centre) pair: entry e has its
 * SpeedCenterDev (n_in, n_out, rows of its clip at that centre) and, in the batch form, a SpeedEntryDev (the clip's
 * pointer, the tables of its key); sub and mags keep one stride per launch, the largest any entry needs.  Descriptors
 * of a pass travel in one copy, its scores come back in one copy behind one synchronisation.  The form selects the
 * kernels (the launchers take the entries or nullptr), nothing else.
 * ------------------------------------------------------------------------------------------------------------------ */
namespace {

std::atomic<size_t> g_speed_batch_bytes { SPEED_BATCH_BYTES };

size_t
align16 (size_t n)
{
  return (n + 15) & ~size_t (15);
}

/* what the first pass asks for per centre of this clip (the clip's length at location 0) */
PassStrides
scan1_strides (size_t n_frames, int n_channels, int rate, const SpeedScanParams& sp)
{
  DeviceWav wav {};
  wav.n_frames = n_frames;
  wav.n_channels = n_channels;
  wav.sample_rate = rate;
  const DeviceWav clip = scan_clip (wav, 0, sp);
  std::vector<ScanCenter> centers;
  append_centers (sp, 1.0, centers);
  PassStrides strides;
  for (ScanCenter& c : centers)
    {
      center_geometry (clip, sp.seconds, c);
      strides.add (c);
    }
  return strides;
}

} // namespace

void
speed_batch_set_bytes (size_t bytes)
{
  g_speed_batch_bytes = bytes ? bytes : SPEED_BATCH_BYTES;
}

size_t
speed_batch_bytes()
{
  return g_speed_batch_bytes;
}

int
speed_batch_plan (const std::vector<size_t>& n_frames, const std::vector<int>& rates, int n_channels, bool patient, size_t budget,
                  std::vector<int>& group_of_clip, std::vector<size_t>& bytes_of_group)
{
  const SpeedScanParams sp = search_plan (patient).scan1;
  const size_t centers = size_t (2 * sp.n_center_steps + 1);
  group_of_clip.assign (n_frames.size(), -1);
  bytes_of_group.clear();
  size_t members = 0;
  PassStrides open;                                        // of the open sub-group
  const auto bytes = [&] (size_t n, const PassStrides& s) {
    return n * centers * (size_t (s.sub_stride (n_channels)) * sizeof (float) + size_t (s.center_stride()) * sizeof (float2));
  };
  for (size_t i = 0; i < n_frames.size(); i++)
    {
      if (!long_enough_to_search (n_frames[i], rates[i]))
        continue;                                          // takes no part in the search
      const PassStrides own = scan1_strides (n_frames[i], n_channels, rates[i], sp);
      PassStrides with = open;
      with.add (own);
      if (members && (bytes (members + 1, with) > budget || members + 1 > SPEED_BATCH_MAX_CLIPS))
        {
          members = 0;                                     // the clip opens the next sub-group (a sub-group holds one clip at least)
          open = PassStrides();
        }
      if (!members)
        bytes_of_group.push_back (0);
      members++;
      open.add (own);
      group_of_clip[i] = int (bytes_of_group.size()) - 1;
      bytes_of_group.back() = bytes (members, open);
    }
  return int (bytes_of_group.size());
}

int
speed_clip_location_batch (awm_ctx *ctx, WorkLane *lane, const std::vector<SpeedBatchItem *>& batch, double seconds, int candidates, SpeedForm form)
{
  (void) ctx;
  SpeedScratch *ws = speed_scratch (lane);
  hipStream_t st = lane->stream;
  if (batch.empty())
    return 0;
  const bool one_clip = form == SpeedForm::ONE_CLIP;       // K15 without descriptors per clip: positions and [n][2] ranges only
  if (one_clip && batch.size() != 1)
    {
      set_error ("speed_clip_location_batch: the one-clip form takes one clip");
      return AWM_ERR_ARG;
    }
  /* get_clip_locations (reference wmspeed.cc:533-553) of every clip: hash a sparse subset of the samples; positions side by side, one gather */
  std::vector<unsigned long long> pos;
  std::vector<awmk::GatherClipDev> gather;
  std::vector<Random> rngs;
  long long max_n = 0;
  for (SpeedBatchItem *item : batch)
    {
      rngs.emplace_back (item->key, 0, Random::Stream::speed_clip);
      Random& rng = rngs.back();
      const size_t first = pos.size(), n_values = item->wav.n_values();
      for (size_t p = 0; p < n_values; p += rng() % 1000)
        pos.push_back (p);
      gather.push_back ({ item->wav.data, (long long) first, (long long) (pos.size() - first) });
      max_n = std::max (max_n, gather.back().n);
    }
  const size_t pos_bytes = align16 (pos.size() * sizeof (unsigned long long)), gather_bytes = one_clip ? 0 : gather.size() * sizeof (awmk::GatherClipDev);
  const size_t val_bytes = pos.size() * sizeof (float);
  const size_t n_ranges = batch.size() * size_t (candidates);
  const size_t range_bytes = n_ranges * (one_clip ? 2 * sizeof (long long) : sizeof (awmk::EnergyRangeDev));
  const size_t e_bytes = n_ranges * awmk::ENERGY_PARTS * sizeof (double);
  if (int rc = ws->gather_pos.reserve (std::max<size_t> (pos_bytes + gather_bytes, 16)))
    return rc;
  if (int rc = ws->gather_out.reserve (std::max<size_t> (val_bytes, 16)))
    return rc;
  if (int rc = ws->ranges.reserve (range_bytes))
    return rc;
  if (int rc = ws->energy.reserve (e_bytes))
    return rc;
  // the staging area holds what goes up and what comes down side by side: no synchronisation between the directions
  if (int rc = ws->pin.reserve (std::max<size_t> (std::max (pos_bytes + gather_bytes + val_bytes, range_bytes + e_bytes), 1 << 16)))
    return rc;
  char *pin = ws->pin.as<char>();
  std::memcpy (pin, pos.data(), pos.size() * sizeof (unsigned long long));
  std::memcpy (pin + pos_bytes, gather.data(), gather_bytes);
  AWM_HIP_CHECK (hipMemcpyAsync (ws->gather_pos.ptr, pin, pos_bytes + gather_bytes, hipMemcpyHostToDevice, st));
  if (one_clip)
    AWM_HIP_CHECK (awmk::launch_gather_values (st, gather[0].in, ws->gather_pos.as<unsigned long long>(), gather[0].n, ws->gather_out.as<float>()));
  else
    AWM_HIP_CHECK (awmk::launch_gather_values_batch (st, reinterpret_cast<const awmk::GatherClipDev *> (ws->gather_pos.as<char>() + pos_bytes), int (gather.size()),
                                                     max_n, ws->gather_pos.as<unsigned long long>(), ws->gather_out.as<float>()));
  const float *values = reinterpret_cast<const float *> (pin + pos_bytes + gather_bytes);
  AWM_HIP_CHECK (hipMemcpyAsync (pin + pos_bytes + gather_bytes, ws->gather_out.ptr, val_bytes, hipMemcpyDeviceToHost, st));
  AWM_HIP_CHECK (hipStreamSynchronize (st));
  std::vector<double> locations;                           // [clip][candidate]
  std::vector<awmk::EnergyRangeDev> ranges;
  for (size_t b = 0; b < batch.size(); b++)
    {
      const DeviceWav& wav = batch[b]->wav;
      unsigned char hash[20];
      sha1 (values + gather[b].first, size_t (gather[b].n) * sizeof (float), hash);          // Random::seed_from_hash (reference random.cc:184-190)
      uint64_t seed = 0;
      for (int i = 0; i < 8; i++)
        seed = (seed << 8) | hash[i];
      rngs[b].seed (seed, Random::Stream::speed_clip);
      for (int c = 0; c < candidates; c++)
        {
          locations.push_back (rngs[b].random_double());
          size_t start_point, end_point;
          speed_clip_range (locations.back(), wav, seconds, &start_point, &end_point);
          ranges.push_back ({ wav.data, (long long) (start_point * wav.n_channels), (long long) (end_point * wav.n_channels) });
        }
    }
  /* get_best_clip_location (reference wmspeed.cc:555-577): the candidate with the highest energy, per clip */
  if (one_clip)
    for (size_t k = 0; k < n_ranges; k++)
      {
        reinterpret_cast<long long *> (pin)[2 * k] = ranges[k].begin;
        reinterpret_cast<long long *> (pin)[2 * k + 1] = ranges[k].end;
      }
  else
    std::memcpy (pin, ranges.data(), range_bytes);
  AWM_HIP_CHECK (hipMemcpyAsync (ws->ranges.ptr, pin, range_bytes, hipMemcpyHostToDevice, st));
  if (one_clip)
    AWM_HIP_CHECK (awmk::launch_energy (st, gather[0].in, ws->ranges.as<long long>(), int (n_ranges), ws->energy.as<double>()));
  else
    AWM_HIP_CHECK (awmk::launch_energy_batch (st, ws->ranges.as<awmk::EnergyRangeDev>(), int (n_ranges), ws->energy.as<double>()));
  AWM_HIP_CHECK (hipMemcpyAsync (pin + range_bytes, ws->energy.ptr, e_bytes, hipMemcpyDeviceToHost, st));
  AWM_HIP_CHECK (hipStreamSynchronize (st));
  const double *parts = reinterpret_cast<const double *> (pin + range_bytes);
  for (size_t b = 0; b < batch.size(); b++)
    {
      double clip_location = 0, best_energy = 0;
      for (int c = 0; c < candidates; c++)
        {
          double energy = 0;
          for (int k = 0; k < awmk::ENERGY_PARTS; k++)
            energy += parts[(b * candidates + c) * awmk::ENERGY_PARTS + k];
          if (energy > best_energy)
            {
              best_energy = energy;
              clip_location = locations[b * candidates + c];
            }
        }
      batch[b]->clip_location = clip_location;
    }
  return 0;
}

int
speed_clip_location (awm_ctx *ctx, WorkLane *lane, const Key& key, const DeviceWav& wav, double seconds, int candidates, double *location)
{
  SpeedBatchItem item;
  item.key = key;
  item.wav = wav;
  if (int rc = speed_clip_location_batch (ctx, lane, { &item }, seconds, candidates, SpeedForm::ONE_CLIP))
    return rc;
  *location = item.clip_location;
  return 0;
}

int
speed_scan_batch (awm_ctx *ctx, WorkLane *lane, const std::vector<SpeedBatchItem *>& batch, const SpeedScanParams& sp, SpeedForm form,
                  SpeedMagsView *mags_view)
{
  SpeedScratch *ws = speed_scratch (lane);
  if (int rc = ensure_window (ctx))
    return rc;
  const bool one_clip = form == SpeedForm::ONE_CLIP;
  if (one_clip && batch.size() != 1)
    {
      set_error ("speed_scan_batch: the one-clip form takes one clip");
      return AWM_ERR_ARG;
    }
  struct Part { SpeedBatchItem *item; DeviceWav clip; SpeedKeyTables *skt; size_t first, count; };
  std::vector<Part> parts;
  std::vector<ScanCenter> centers;                         // of all clips, clip after clip
  std::vector<double> ratios;
  int C = 0;
  for (SpeedBatchItem *item : batch)
    {
      item->scores.clear();
      if (item->rc || item->speeds.empty())
        continue;
      Part part { item, item->wav, nullptr, centers.size(), 0 };
      for (double speed : item->speeds)
        append_centers (sp, speed, centers);
      for (size_t i = part.first; i < centers.size() && !item->rc; i++)
        if (!var_geometry (centers[i].speed / 2).ok)       // the clip drops out, the others go on (not set_error: the call goes on)
          {
            item->error = string_printf ("failed to setup vresampler with ratio=%f", centers[i].speed / 2);
            item->rc = AWM_ERR_ARG;
          }
      if (item->rc)
        {
          centers.resize (part.first);
          continue;
        }
      if (C && item->wav.n_channels != C)
        {
          set_error ("speed_scan_batch: the clips of a launch have one channel count");
          return AWM_ERR_ARG;
        }
      C = item->wav.n_channels;
      part.clip = scan_clip (item->wav, item->clip_location, sp);
      part.count = centers.size() - part.first;
      part.skt = get_speed_key_tables (ctx, item->key);    // (never evicted: alive for the launches below)
      if (!part.skt)
        return AWM_ERR_HIP;
      parts.push_back (part);
    }
  if (centers.empty())
    return 0;
  if (centers.size() > SPEED_BATCH_MAX_ENTRIES)
    {
      set_error ("speed_scan_batch: too many (clip, centre) pairs for one launch");
      return AWM_ERR_ARG;
    }
  // every ratio once (the first pass has the same 57 for every clip): the lookup below runs under the context's table lock
  std::vector<double> unique_ratios;
  std::vector<size_t> table_of;
  {
    std::map<double, size_t> seen;
    for (const auto& c : centers)
      {
        ratios.push_back (c.speed / 2);
        const auto it = seen.emplace (ratios.back(), unique_ratios.size());
        if (it.second)
          unique_ratios.push_back (ratios.back());
        table_of.push_back (it.first->second);
      }
  }
  std::vector<VarResampleTable *> unique_tables, tables;
  if (int rc = get_var_tables (ctx, unique_ratios, unique_tables))
    return rc;
  for (size_t t : table_of)
    tables.push_back (unique_tables[t]);
  const int per = 2 * sp.n_steps + 1;
  std::vector<awmk::SpeedCenterDev> cds;
  std::vector<awmk::SpeedEntryDev> entries;
  std::vector<awmk::SpeedItemDev> items;
  std::vector<double> item_speed;
  PassStrides strides;
  bool aligned = true;
  awmk::VarResampleArgs ra {};
  double var_bytes = 0, mags_bytes = 0, compare_bytes = 0;
  for (const Part& part : parts)
    {
      aligned = aligned && (reinterpret_cast<uintptr_t> (part.clip.data) & 7) == 0;
      for (size_t i = part.first; i < part.first + part.count; i++)
        {
          ScanCenter& c = centers[i];
          c.table = tables[i];
          center_geometry (part.clip, sp.seconds, c);
          awmk::SpeedCenterDev cd = center_dev (c.table, ratios[i], c.n_in, c.n_out);
          cd.rows = c.rows;
          cds.push_back (cd);
          entries.push_back ({ part.clip.data, part.skt->cols.as<unsigned int>(), part.skt->col_frame.as<int>(), part.skt->col_first.as<unsigned char>() });
          strides.add (c);
          ra.max_stride = std::max (ra.max_stride, cd.stride);
          ra.max_step = std::max (ra.max_step, std::ldexp (double (cd.mant), -cd.shift));
          var_bytes += double (c.n_in + c.n_out) * C * 4.0;                   // K12: the clip in, the resampled clip out, per centre speed
          mags_bytes += double (c.n_out) * C * 4.0 + double (c.rows) * 510 * 8.0;   // K13: the resampled clip once, { umag, dmag } per row and sync frame out
          // K14: every centre's { umag, dmag } matrix once (its 2 n_steps + 1 relative speeds share it) + one best score per item
          compare_bytes += double (c.rows) * 510 * 8.0 + per * 8.0;
          /* SpeedSync::get_jobs (reference wmspeed.cc:172-192): relative speeds step^p, p = -n_steps .. n_steps, per centre */
          for (int p = -sp.n_steps; p <= sp.n_steps; p++)
            {
              const double center = c.speed;
              const double relative_speed = std::pow (sp.step, p) * center / center;
              awmk::SpeedItemDev it {};
              it.center = int (i);
              it.rel_speed_inv = 1 / relative_speed;
              it.q16_scale = (1 << 16) / relative_speed;
              items.push_back (it);
              item_speed.push_back (relative_speed * center);
            }
        }
    }
  const long long ld = strides.ld(), sub_stride = strides.sub_stride (C), center_stride = strides.center_stride();
  const size_t n = centers.size();
  // one blob of descriptors: centres, entries (batch form only), items
  const size_t cds_bytes = align16 (n * sizeof (awmk::SpeedCenterDev)), entries_bytes = one_clip ? 0 : align16 (n * sizeof (awmk::SpeedEntryDev));
  const size_t items_bytes = align16 (items.size() * sizeof (awmk::SpeedItemDev)), best_bytes = items.size() * sizeof (unsigned long long);
  const size_t blob_bytes = cds_bytes + entries_bytes + items_bytes;
  if (int rc = ws->sub.reserve (std::max<size_t> (size_t (sub_stride) * n * sizeof (float), 16)))
    return rc;
  if (int rc = ws->mags.reserve (std::max<size_t> (size_t (center_stride) * n * sizeof (float2), 16)))
    return rc;
  if (int rc = ws->centers.reserve (blob_bytes))
    return rc;
  if (int rc = ws->best.reserve (best_bytes))
    return rc;
  if (int rc = ws->pin.reserve (std::max<size_t> (blob_bytes + best_bytes, 1 << 16)))
    return rc;
  hipStream_t st = lane->stream;
  char *pin = ws->pin.as<char>(), *dev = ws->centers.as<char>();
  std::memcpy (pin, cds.data(), n * sizeof (awmk::SpeedCenterDev));
  if (!one_clip)
    std::memcpy (pin + cds_bytes, entries.data(), n * sizeof (awmk::SpeedEntryDev));
  std::memcpy (pin + cds_bytes + entries_bytes, items.data(), items.size() * sizeof (awmk::SpeedItemDev));
  AWM_HIP_CHECK (hipMemcpyAsync (dev, pin, blob_bytes, hipMemcpyHostToDevice, st));
  const awmk::SpeedCenterDev *cds_d = reinterpret_cast<const awmk::SpeedCenterDev *> (dev);
  // The form: with entries the launchers take the batch kernels, with nullptr the one-clip kernels, which read the clip and the key's
  // tables from the args (those of the one part; the batch kernels do not look at them)
  const awmk::SpeedEntryDev *entries_d = one_clip ? nullptr : reinterpret_cast<const awmk::SpeedEntryDev *> (dev + cds_bytes);
  ra.in = entries[0].in;
  ra.n_channels = C;
  ra.centers = cds_d;
  ra.out = ws->sub.as<float>();
  ra.out_stride = sub_stride;
  {
    ProfScope ps (ctx, PROF_RESAMPLE_VAR, var_bytes, st);
    AWM_HIP_CHECK (awmk::launch_resample_var (st, ra, strides.max_out, int (n), entries_d, aligned));
  }
  awmk::SpeedMagsArgs ma {};
  ma.sub = ws->sub.as<float>();
  ma.sub_stride = sub_stride;
  ma.n_channels = C;
  ma.centers = cds_d;
  ma.window512 = workspace (ctx)->window512.as<float>();        // (built by ensure_window above; never replaced)
  ma.cols = entries[0].cols;
  ma.mags = ws->mags.as<float2>();
  ma.mags_center_stride = center_stride;
  ma.ld = ld;
  {
    ProfScope ps (ctx, PROF_SPEED_MAGS, mags_bytes, st);
    AWM_HIP_CHECK (awmk::launch_speed_mags (st, ctx->tabs, ma, strides.max_rows, int (n), entries_d));
  }
  if (mags_view)                                           // the test view of the matrices: no comparison
    {
      AWM_HIP_CHECK (hipStreamSynchronize (st));
      mags_view->ld = ld;
      mags_view->rows = centers[0].rows;
      return 0;
    }
  AWM_HIP_CHECK (hipMemsetAsync (ws->best.ptr, 0, best_bytes, st));
  const int steps_per_frame = Params::frame_size / Params::sync_search_step;
  const int frames_per_block = int (mark_block_frame_count());
  awmk::SpeedCompareArgs ca {};
  ca.mags = ws->mags.as<float2>();
  ca.mags_center_stride = center_stride;
  ca.ld = ld;
  ca.centers = cds_d;
  ca.items = reinterpret_cast<const awmk::SpeedItemDev *> (dev + cds_bytes + entries_bytes);
  ca.n_centers = int (n);
  ca.items_per_center = per;
  ca.col_frame = entries[0].col_frame;
  ca.col_first = entries[0].col_first;
  ca.frames_per_block = frames_per_block;
  ca.steps_per_frame = steps_per_frame;
  ca.pad_start = frames_per_block * steps_per_frame + steps_per_frame;      // "a bit of overlap to handle boundaries"
  ca.rows_per_bit = Params::sync_frames_per_bit;
  ca.min_delta = std::min (params().water_delta, 0.080);
  ca.best = ws->best.as<unsigned long long>();
  {
    ProfScope ps (ctx, PROF_SPEED_COMPARE, compare_bytes, st);
    AWM_HIP_CHECK (awmk::launch_speed_compare (st, ca, int (items.size()), entries_d));
  }
  AWM_HIP_CHECK (hipMemcpyAsync (pin + blob_bytes, ws->best.ptr, best_bytes, hipMemcpyDeviceToHost, st));
  AWM_HIP_CHECK (hipStreamSynchronize (st));
  const double *best = reinterpret_cast<const double *> (pin + blob_bytes);
  for (const Part& part : parts)
    for (size_t i = part.first * per; i < (part.first + part.count) * per; i++)
      {
        SpeedScore sc;                                     // "Score best_score": stays { 0, 0 } unless a state has quality > 0
        if (best[i] > 0)
          {
            sc.quality = best[i];
            sc.speed = item_speed[i];
          }
        part.item->scores.push_back (sc);
      }
  return 0;
}

int
speed_scan (awm_ctx *ctx, WorkLane *lane, const Key& key, const DeviceWav& wav, double clip_location, const SpeedScanParams& sp,
            const std::vector<double>& speeds, std::vector<SpeedScore>& scores, SpeedMagsView *mags_view)
{
  SpeedBatchItem item;
  item.key = key;
  item.wav = wav;
  item.clip_location = clip_location;
  item.speeds = speeds;
  if (int rc = speed_scan_batch (ctx, lane, { &item }, sp, SpeedForm::ONE_CLIP, mags_view))
    return rc;
  if (item.rc)
    {
      set_error (item.error);
      return item.rc;
    }
  scores = item.scores;
  return 0;
}

int
speed_mags (awm_ctx *ctx, WorkLane *lane, const Key& key, const DeviceWav& wav, double clip_location, double center, double seconds,
            std::vector<float>& out, int *rows)
{
  SpeedScratch *ws = speed_scratch (lane);
  std::vector<SpeedScore> scores;
  SpeedMagsView view;
  if (int rc = speed_scan (ctx, lane, key, wav, clip_location, { seconds, 1.0, 0, 0 }, { center }, scores, &view))   // (the centre itself: step^0)
    return rc;
  const long long ld = view.ld;
  KeyTables *kt = ctx->get_key_tables (key);
  const SyncTable& stab = kt->sync[0].host;
  std::vector<float2> m (size_t (510) * ld);
  AWM_HIP_CHECK (hipMemcpy (m.data(), ws->mags.ptr, m.size() * sizeof (float2), hipMemcpyDeviceToHost));
  // back to the reference's column order (all 510 sync frames sorted by frame)
  std::vector<int> order (510);
  for (int i = 0; i < 510; i++)
    order[i] = i;
  std::sort (order.begin(), order.end(), [&] (int a, int b) { return stab.frame[a] < stab.frame[b]; });
  *rows = view.rows;
  out.assign (size_t (*rows) * 510 * 2, 0.f);
  for (int r = 0; r < *rows; r++)
    for (int c = 0; c < 510; c++)
      {
        const float2 v = m[size_t (order[c]) * ld + r];
        out[(size_t (r) * 510 + c) * 2] = v.x;
        out[(size_t (r) * 510 + c) * 2 + 1] = v.y;
      }
  return 0;
}

namespace {

/* run_search (reference wmspeed.cc:622-781) for the clips of `batch` in lockstep: clip location, scan 1, the n best, scan 2, the best,
 * scan 3, smoothing and thresholds.  A clip whose scores run empty or whose search fails drops out, the others go on. */
int
speed_search (awm_ctx *ctx, WorkLane *lane, const std::vector<SpeedBatchItem *>& batch, const SearchPlan& plan, SpeedForm form,
              std::vector<SpeedBatchResult>& results)
{
  results.assign (batch.size(), SpeedBatchResult());
  if (int rc = speed_clip_location_batch (ctx, lane, batch, plan.scan1.seconds, clip_candidates, form))
    return rc;
  for (SpeedBatchItem *item : batch)
    item->speeds = { 1.0 };
  if (int rc = speed_scan_batch (ctx, lane, batch, plan.scan1, form))
    return rc;
  for (SpeedBatchItem *item : batch)
    {
      select_n_best_scores (item->scores, plan.n_best);
      item->speeds.clear();
      for (const auto& s : item->scores)
        item->speeds.push_back (s.speed);
    }
  if (int rc = speed_scan_batch (ctx, lane, batch, plan.scan2, form))
    return rc;
  for (SpeedBatchItem *item : batch)
    {
      select_n_best_scores (item->scores, 1);
      item->speeds.clear();
      if (!item->scores.empty())                           // (empty: the clip takes no part in the last pass, it stays unsearched)
        item->speeds.push_back (item->scores[0].speed);
    }
  if (int rc = speed_scan_batch (ctx, lane, batch, plan.scan3, form))
    return rc;
  for (size_t b = 0; b < batch.size(); b++)
    {
      const SpeedBatchItem& item = *batch[b];
      SpeedBatchResult& r = results[b];
      r.rc = item.rc;
      r.error = item.error;
      if (item.rc || item.speeds.empty())
        continue;
      r.searched = true;
      r.speed = score_smooth_find_best (item.scores, 1 - plan.scan3.step, scan3_smooth_distance);
      for (const auto& s : item.scores)
        r.quality = std::max (r.quality, s.quality);
      // "speeds closer to 1.0 than this usually work without stretching before decode"
      r.use = r.quality > speed_sync_threshold && (r.speed < 0.9999 || r.speed > 1.0001);
    }
  return 0;
}

} // namespace

int
detect_speed (awm_ctx *ctx, WorkLane *lane, const std::vector<Key>& key_list, const DeviceWav& wav, std::string *report,
              std::vector<DetectSpeedResult>& results, double *best_speed_out, double *best_quality_out)
{
  results.clear();
  if (!long_enough_to_search (wav.n_frames, wav.sample_rate))
    return 0;
  const SearchPlan plan = search_plan (params().detect_speed_patient);
  for (const Key& key : key_list)                          // key after key, each a search of one clip
    {
      SpeedBatchItem item;
      item.key = key;
      item.wav = wav;
      std::vector<SpeedBatchResult> found;
      if (int rc = speed_search (ctx, lane, { &item }, plan, SpeedForm::ONE_CLIP, found))
        return rc;
      const SpeedBatchResult& r = found[0];
      if (r.rc)
        {
          set_error (r.error);
          return r.rc;
        }
      if (!r.searched)
        continue;
      if (report)
        {
          double delta = -1;
          if (params().test_speed > 0)
            delta = 100 * std::fabs (r.speed - params().test_speed) / params().test_speed;
          *report += string_printf ("detect_speed %f %f %.4f\n", r.speed, r.quality, delta);
        }
      if (best_speed_out)
        *best_speed_out = r.speed;
      if (best_quality_out)
        *best_quality_out = r.quality;
      if (r.use)
        results.push_back ({ key, r.speed });
    }
  return 0;
}

int
detect_speed_batch (awm_ctx *ctx, WorkLane *lane, const std::vector<SpeedBatchClip>& clips, std::vector<SpeedBatchResult>& results)
{
  results.assign (clips.size(), SpeedBatchResult());
  if (clips.empty())
    return 0;
  std::vector<size_t> n_frames;
  std::vector<int> rates, group;
  std::vector<size_t> group_bytes;
  for (const auto& c : clips)
    {
      if (c.wav.n_channels != clips[0].wav.n_channels)
        {
          set_error ("detect_speed_batch: the clips of a batch have one channel count");
          return AWM_ERR_ARG;
        }
      n_frames.push_back (c.wav.n_frames);
      rates.push_back (c.wav.sample_rate);
    }
  /* a clip too short to search is in no sub-group */
  const int n_groups = speed_batch_plan (n_frames, rates, clips[0].wav.n_channels, params().detect_speed_patient, speed_batch_bytes(), group, group_bytes);
  const SearchPlan plan = search_plan (params().detect_speed_patient);
  std::vector<SpeedBatchItem> items (clips.size());
  for (int g = 0; g < n_groups; g++)
    {
      std::vector<SpeedBatchItem *> batch;
      std::vector<size_t> clip_of;
      for (size_t i = 0; i < clips.size(); i++)
        if (group[i] == g)
          {
            items[i].key = clips[i].key;
            items[i].wav = clips[i].wav;
            batch.push_back (&items[i]);
            clip_of.push_back (i);
          }
      std::vector<SpeedBatchResult> found;
      if (int rc = speed_search (ctx, lane, batch, plan, SpeedForm::BATCH, found))
        return rc;
      for (size_t b = 0; b < batch.size(); b++)
        results[clip_of[b]] = found[b];
    }
  return 0;
}

} // namespace awm
