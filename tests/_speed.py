"""The speed detection kernels (K12 .. K14: csrc/hip/speed.hip) restated in plain numpy, and the material that sits on their special
cases.  TEST INFRASTRUCTURE ONLY; no GPU.  Built on tests/_sliding.py (ulp32, _db64, K_ULPS, DB_FACTOR).

var_resample32() is K12's arithmetic in float32 on the product's own coefficient table (audiowmark_amd.binding.var_resample_table):
the phase of output m from the exact product m * mant >> shift in Python integers, the fraction as float64 (frac) * frac_scale with
the round-up to a whole step where that product reaches 256, then zita's sums c1 = a q1[i] + b q1[i + hl], c2 = a q2[i] + b q2[i - hl],
s = s + (x1 c1 + x2 c2) with every product and sum rounded to float32, from 1e-25f, which is taken off again at the end; zeros outside
[0, n_in).  K12 is held to it BIT FOR BIT.  zita_phases() is the accumulated phase of zita's VResampler (ph += step in double with
wrap), which the oracle runs: the two give the same (window, k, bf) for all but a small share of the outputs, see PHASE_SHARE.

The round-up branch (ph >= 256).  The fraction has `shift` bits; float64 (frac) rounds up to 2^shift only for the topmost
2^(shift - 54) values of frac, and shift = 61 - e with step = 256 / ratio = f 2^e: shift <= 53 (no rounding at all) for every ratio
<= 2.  Above 2 it fires where m * mant lands on one of those residues: first_round_up() solves m * mant = frac (mod 2^shift) for the
smallest such m.  At 2.5 and 7.3 there is none (an even mantissa, odd residues); at generic ratios it lies beyond 2^40 outputs; at
3.0 the step is 256 / 3 rounded down and output 3 (3 step = 256 - 2^-46, which is 256 in a double) rounds up -- the ratio at which the
GPU test runs the branch, asserting from the restatement that it fired there and nowhere else.

mags64() is what K13 claims to compute: numpy's float64 rfft of the 512 samples at 128 row of the half-rate clip, weighted by the
analytic von Hann window, bins 20..100, then the reference's last float steps as _frames.channel_frames does them (re and im rounded
to float32, the float32 abs2, abs2 > 0 ? log2 (abs2) * 3.01029995663981f : -96), the channels added in float32 in channel order, and
the 30 up / 30 down bands of each of the 510 sync frames added in float32 in table order.  A channel whose 512 samples are all zero
gives exactly -96 per band.
THE TOLERANCE is derived per value.  K13 carries two channels in the real and imaginary part of ONE complex float32 FFT-512, so re
and im of either channel carry an absolute error of about eps32 times the norm of the PAIR:
    delta = K_FFT512 eps32 ||(x0 w, x1 w)||_2      (a single channel -- mono, the third of three -- its own norm)
    tol (band) = sum over the channels of the sensitivity to +-delta on re and im + K_ULPS ulp32 (|value|)
    tol (column) = sum of its 30 bands' tol + 30 ulp32 (largest running sum)
and 0 where the silence rule fires in every channel.  K_FFT512 is measured, never against the kernels: test_speed_restated.py takes
the largest |X32 - X64| / (eps32 ||x w||_2) of scipy's float32 rfft over the rows of every material below (OBSERVED_FFT512 there);
the kernel gets twice the largest, as K4 does.

compare() is K14 restated from SpeedSync::compare (oracle/awm_oracle.cc): states -pad_start .. -1, offsets and frame offsets Q16 in
64 bits, float32 sums per sync bit in the order block 0, 1, 2 and frame ascending, odd blocks swapping up and down; bit_quality in
float32, the weighting by the counts and the normalisation in double.  Vectorised over the states, per column; the run of states that
sees a column comes from the monotonic bounds.  K14 is held to it BIT FOR BIT on K13's own matrices."""
import math

import numpy as np

from _sliding import DB_FACTOR, K_ULPS, MAX_BAND, MIN_BAND, NB, _db64, ulp32  # noqa: F401  (re-exported)

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23
NP = 256                                         # phases of the VResampler's table
N512, HOP = 512, 128                             # K13: transform size and hop at half rate
SYNC_COLS = 510
FRAMES_PER_BLOCK, STEPS_PER_FRAME = 2226, 4
PAD_START = FRAMES_PER_BLOCK * STEPS_PER_FRAME + STEPS_PER_FRAME
WINDOW512 = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N512) / N512)) / 128          # float64
# twice the largest of test_speed_restated.py's OBSERVED_FFT512 (that test asserts the equation)
K_FFT512 = 2 * 13.1
# share of outputs for which zita's accumulated phase and the exact product give another (window, k, bf), 100 000 outputs per ratio
# (20 000 at 1 / 16), measured on 2026-10-21 (test_speed_restated.py prints it and asserts < 1 %): the largest over its generic ratios
# 0.49, 1 / 1.01, 1 / 0.9764, 0.8, 7.3, 1 / 16.  (Ratios whose step is a short fraction of 256 are another matter: see that file.)
PHASE_SHARE = 0.0


# ---- K12 -----------------------------------------------------------------------------------------------------------------------------
class VarGeometry:
    """VResampler::setup (ratio, nchan, 16) as the closed form the kernel uses: output m reads the window that starts at input frame
    (m * mant >> shift) - (hl - 1); step = 256 / ratio = mant 2^-53 2^e, shift = 61 - e"""
    def __init__(self, ratio):
        if not (16 * ratio >= 1) or ratio > 256:
            raise ValueError("ratio %r refused" % ratio)
        self.ratio = ratio
        self.hl, self.frel = 16, 1.0 - 2.6 / 16
        if ratio < 1:
            self.frel *= ratio
            self.hl = int(math.ceil(16 / ratio))
        self.step = 256 / ratio
        f, e = math.frexp(self.step)
        self.mant = int(math.ldexp(f, 53))
        self.shift = 61 - e
        self.frac_scale = math.ldexp(1.0, e - 53)
        assert self.mant * self.frac_scale == self.step          # (the step is the double itself)


def zita_table64(geo):
    """the dense [257][hl] table of zita's Resampler_table::create in float64 (not yet rounded to float32)"""
    hl = geo.hl
    t = np.arange(NP + 1)[:, None] / float(NP) + np.arange(hl)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.abs(t * geo.frel)
        sinc = np.where(x < 1e-6, 1.0, np.sin(x * np.pi) / (x * np.pi))
        y = np.abs(t / hl)
        wind = np.where(y >= 1.0, 0.0, 0.384 + 0.500 * np.cos(y * np.pi) + 0.116 * np.cos(2 * (y * np.pi)))
    return np.ascontiguousarray((geo.frel * sinc * wind)[:, ::-1])          # p[hl - i - 1] = value at t = j / np + i


def var_phase(geo, m):
    """(whole input frames b, phase k, fraction bf float32, the round-up fired) of output m, as var_phase() in speed.hip"""
    prod = int(m) * geo.mant
    b, frac = prod >> geo.shift, prod & ((1 << geo.shift) - 1)
    ph = float(frac) * geo.frac_scale
    fired = ph >= NP
    if fired:
        ph, b = 0.0, b + 1
    k = int(ph)
    return b, k, np.float32(ph - k), fired


def var_phases(geo, outputs):
    """var_phase for a list of outputs: (b int64 [n], k int64 [n], bf float32 [n], fired bool [n])"""
    ph = [var_phase(geo, m) for m in outputs]
    return (np.array([p[0] for p in ph], np.int64), np.array([p[1] for p in ph], np.int64), np.array([p[2] for p in ph], np.float32),
            np.array([p[3] for p in ph], bool))


def zita_phases(geo, n_out):
    """(b, k, bf) of the outputs 0 .. n_out - 1 with zita's accumulated phase (VResampler::process: ph += step; on ph >= 256 the
    window moves by floor (ph / 256) frames)"""
    b = np.empty(n_out, np.int64)
    k = np.empty(n_out, np.int64)
    bf = np.empty(n_out, np.float32)
    ph, frames, step = 0.0, 0, geo.step
    for m in range(n_out):
        kk = int(ph)
        b[m], k[m], bf[m] = frames, kk, np.float32(ph - kk)
        ph += step
        if ph >= NP:
            nr = int(math.floor(ph / NP))
            ph -= nr * NP
            frames += nr
    return b, k, bf


def first_round_up(geo):
    """the smallest output m >= 0 for which var_phase's round-up fires (None if it cannot: shift <= 53, or no solution)"""
    if geo.shift <= 53:
        return None
    mod = 1 << geo.shift
    best = None
    for frac in range(mod - (1 << (geo.shift - 54)), mod):
        assert float(frac) * geo.frac_scale >= NP and float(frac - (1 << (geo.shift - 54))) * geo.frac_scale < NP
        g = math.gcd(geo.mant, mod)
        if frac % g:
            continue
        m = (frac // g) * pow(geo.mant // g, -1, mod // g) % (mod // g)
        assert (m * geo.mant) % mod == frac
        best = m if best is None else min(best, m)
    return best


def _taps(x, table, hl, b, k, bf):
    n_in, C = x.shape
    a = np.float32(1) - bf
    first = b - (hl - 1)
    s = np.full((len(b), C), np.float32(1e-25), np.float32)
    for i in range(hl):
        c1 = a * table[k, i] + bf * table[k + 1, i]
        c2 = a * table[NP - k, i] + bf * table[NP - k - 1, i]
        j1, j2 = first + i, first + 2 * hl - 1 - i
        ok1, ok2 = (j1 >= 0) & (j1 < n_in), (j2 >= 0) & (j2 < n_in)
        x1 = np.where(ok1[:, None], x[np.where(ok1, j1, 0)], np.float32(0))
        x2 = np.where(ok2[:, None], x[np.where(ok2, j2, 0)], np.float32(0))
        s = s + (x1 * c1[:, None] + x2 * c2[:, None])
    assert s.dtype == np.float32 and c1.dtype == np.float32
    return s - np.float32(1e-25)


def var_resample32(x, table, hl, ratio, n_out, outputs=None, phases=None, info=None):
    """the outputs `outputs` (default: all of 0 .. n_out - 1) of K12 for the input x [n_in][C] float32 -> [len (outputs)][C] float32.
    phases = (b, k, bf) replaces the exact-product phase (zita_phases); info (a dict) receives the number of round-ups"""
    x = np.asarray(x, np.float32)
    table = np.asarray(table, np.float32)
    geo = VarGeometry(ratio)
    assert x.ndim == 2 and table.shape == (NP + 1, hl) and hl == geo.hl
    if outputs is None:
        outputs = np.arange(n_out, dtype=np.int64)
    outputs = np.asarray(outputs, np.int64)
    assert len(outputs) == 0 or (outputs.min() >= 0 and outputs.max() < n_out)
    if phases is None:
        b, k, bf, fired = var_phases(geo, outputs.tolist())
        if info is not None:
            info["round_ups"] = int(fired.sum())
    else:
        b, k, bf = (p[outputs] for p in phases)
    out = np.empty((len(outputs), x.shape[1]), np.float32)
    with np.errstate(under="ignore"):
        for o in range(0, len(outputs), 1 << 16):
            sl = slice(o, o + (1 << 16))
            out[sl] = _taps(x, table, hl, b[sl], k[sl], bf[sl])
    return out


def resample_frames(n_frames, ratio):
    """frames resample_ratio_truncate produces (lrint: ties to even)"""
    return int(round(n_frames * ratio))


# ---- K13 -----------------------------------------------------------------------------------------------------------------------------
def key_cols(key):
    """the 510 sync frames of a block in the reference's column order (sorted by frame): dict of bit [510], frame [510], up [510][30],
    down [510][30] (bands 0..80), from the oracle's sync table"""
    import _oracle as orc
    t = orc.sync_bits(key).reshape(6 * 85, 61)
    bit = np.repeat(np.arange(6), 85)
    order = np.argsort(t[:, 0], kind="stable")
    assert len(np.unique(t[:, 0])) == SYNC_COLS
    return dict(bit=bit[order], frame=t[order, 0].astype(np.int64), up=t[order, 1:31], down=t[order, 31:61])


def rows_of(n_out):
    """time steps of prepare_mags: pos + 512 < n_out, pos = 0, 128, ..."""
    return (n_out - N512 - 1) // HOP + 1 if n_out > N512 else 0


def spectrum512(sub, c, rows):
    """(X [rows][81] complex128 of the windowed rows of channel c, ||x w||_2 [rows], dead [rows]: the 512 samples are all zero)"""
    idx = HOP * np.arange(rows)[:, None] + np.arange(N512)[None, :]
    fr = sub[idx, c]
    xw = fr.astype(np.float64) * WINDOW512
    return np.fft.rfft(xw, axis=1)[:, MIN_BAND:MAX_BAND + 1], np.sqrt((xw * xw).sum(axis=1)), ~(fr != 0).any(axis=1)


def db_rows(sub, k_fft=None, packed=True):
    """(db [rows][81] float32: the channel sum, tol [rows][81] float64) of the clip sub [n_out][C] float32 at half rate; packed:
    channels 2 i and 2 i + 1 share a transform (the tolerance of either takes the pair's norm)"""
    k_fft = K_FFT512 if k_fft is None else k_fft
    sub = np.asarray(sub, np.float32)
    n_out, C = sub.shape
    rows = rows_of(n_out)
    total = np.zeros((rows, NB), np.float32)
    tol = np.zeros((rows, NB), np.float64)
    all_dead = np.ones(rows, bool)
    parts = [spectrum512(sub, c, rows) for c in range(C)]
    for c in range(C):
        spect, norm, dead = parts[c]
        mate = c ^ 1
        if packed and mate < C:
            norm = np.sqrt(norm * norm + parts[mate][1] ** 2)
        delta = (k_fft * EPS32 * norm)[:, None]
        re, im = spect.real.astype(np.float32), spect.imag.astype(np.float32)
        sens = np.zeros((rows, NB), np.float64)
        with np.errstate(under="ignore"):
            l2, abs2 = _db64(re, im)
            v = np.where(abs2 > 0, l2.astype(np.float32) * DB_FACTOR, np.float32(-96)).astype(np.float32)
            exact = np.where(abs2 > 0, l2 * float(DB_FACTOR), -96.0)
            for sr in (-1, 1):
                for si in (-1, 1):
                    l2p, abs2p = _db64((re.astype(np.float64) + sr * delta).astype(np.float32), (im.astype(np.float64) + si * delta).astype(np.float32))
                    sens = np.maximum(sens, np.abs(np.where(abs2p > 0, l2p * float(DB_FACTOR), -96.0) - exact))
            reach0 = (np.abs(re) <= delta) & (np.abs(im) <= delta)              # abs2 can reach 0 under the perturbation: the -96 branch
            sens = np.where(reach0, np.maximum(sens, np.abs(-96.0 - exact)), sens)
        v[dead] = np.float32(-96)
        sens[dead] = 0
        total = total + v                                        # 0 + db0 + db1 + ..., each a float32 addition
        tol += sens
        all_dead &= dead
    assert total.dtype == np.float32
    tol += K_ULPS * ulp32(total)
    tol[all_dead] = 0
    return total, tol


def column_sums(db, tol, cols):
    """umag / dmag of the 510 sync frames: (mags [rows][510][2] float32, tol alike float64)"""
    rows = db.shape[0]
    mags = np.zeros((rows, SYNC_COLS, 2), np.float32)
    out_tol = np.zeros((rows, SYNC_COLS, 2), np.float64)
    for side, bands in enumerate((cols["up"], cols["down"])):
        s = np.zeros((rows, SYNC_COLS), np.float32)
        t = np.zeros((rows, SYNC_COLS), np.float64)
        running = np.zeros((rows, SYNC_COLS), np.float32)
        exact = np.ones((rows, SYNC_COLS), bool)
        for i in range(30):
            s = s + db[:, bands[:, i]]
            t += tol[:, bands[:, i]]
            exact &= tol[:, bands[:, i]] == 0
            running = np.maximum(running, np.abs(s))
        assert s.dtype == np.float32
        mags[:, :, side] = s
        out_tol[:, :, side] = np.where(exact, 0.0, t + 30 * ulp32(running))      # (sums of -96 C are exact in float32)
    return mags, out_tol


def mags64(sub, cols, k_fft=None, packed=True):
    """K13 as a float64 transform: (mags [rows][510][2] float32, tol alike) of the half-rate clip sub [n_out][C] float32"""
    db, tol = db_rows(sub, k_fft, packed)
    return column_sums(db, tol, cols)


def clip_range(location, n_frames, clip_seconds, rate=44100):
    """get_speed_clip (wmspeed.cc:33-52): (start, end) in frames"""
    end_sec = float(n_frames) / rate
    start_sec = location * (end_sec - clip_seconds)
    if start_sec < 0:
        start_sec = 0
    start = int(start_sec * rate)
    return start, min(int(start + clip_seconds * rate), n_frames)


def mags_geometry(n_frames, location, center, seconds, rate=44100):
    """prepare_mags' own formula: (clip start, input frames, outputs, rows) of one centre speed of a scan over `seconds`"""
    start, end = clip_range(location, n_frames, seconds * 1.3, rate)
    in_frames = end - start
    max_in = seconds / center
    if max_in > 0:
        in_frames = min(in_frames, int(round(rate * max_in)))
    n_out = int(round(in_frames * (center / 2)))
    return start, in_frames, n_out, rows_of(n_out)


def seconds_for_rows(rows, center, extra=0, rate=44100):
    """a `seconds` for which prepare_mags builds exactly `rows` rows at `center` (extra: outputs beyond the last row's window), found
    with the formula itself"""
    want_out = N512 + HOP * (rows - 1) + 1 + extra if rows > 0 else N512 - 3
    for in_frames in range(int(want_out * 2 / center) - 4, int(want_out * 2 / center) + 8):
        seconds = (in_frames + 0.25) * center / rate
        if int(round(rate * (seconds / center))) == in_frames and int(round(in_frames * (center / 2))) == want_out:
            assert rows_of(want_out) == rows
            return seconds
    raise AssertionError("no length gives %d rows at %r" % (rows, center))


# ---- K14 -----------------------------------------------------------------------------------------------------------------------------
def compare(mags, rows, rel_speeds, min_delta, cols, stats=None):
    """SpeedSync::compare for every relative speed on the matrix mags [rows][510][2] float32 (columns sorted by frame): the best
    normalised quality over the states per relative speed, float64 [len (rel_speeds)]; 0 where no state scores (the caller reports
    speed 0 there).  stats (a dict) receives per relative speed the number of (state, column) contributions of blocks 0, 1, 2"""
    mags = np.asarray(mags)
    assert mags.dtype == np.float32 and mags.shape == (rows, SYNC_COLS, 2)
    bit, frame = cols["bit"], cols["frame"]
    best = np.zeros(len(rel_speeds), np.float64)
    for r, rs in enumerate(rel_speeds):
        rs_inv = 1 / rs
        offs = np.trunc(np.arange(-PAD_START, 0) * ((1 << 16) / rs)).astype(np.int64)
        assert (np.diff(offs) >= 0).all()
        u = np.zeros((PAD_START, 6), np.float32)
        d = np.zeros((PAD_START, 6), np.float32)
        n = np.zeros((PAD_START, 6), np.int64)
        counts = [0, 0, 0]
        for block in range(3):
            for mi in range(SYNC_COLS):
                fo = int(((block * FRAMES_PER_BLOCK + int(frame[mi])) * STEPS_PER_FRAME * rs_inv + 0.5) * (1 << 16))
                lo = int(np.searchsorted(offs, -fo, "left"))                    # offset + frame_offset >= 0
                hi = int(np.searchsorted(offs, (rows << 16) - fo, "left"))      # (offset + frame_offset) >> 16 < rows
                if lo >= hi:
                    continue
                idx = (offs[lo:hi] + fo) >> 16
                uu, dd = mags[idx, mi, 0], mags[idx, mi, 1]
                if block & 1:
                    uu, dd = dd, uu
                u[lo:hi, bit[mi]] += uu
                d[lo:hi, bit[mi]] += dd
                n[lo:hi, bit[mi]] += 1
                counts[block] += hi - lo
        assert u.dtype == np.float32
        q = np.zeros(PAD_START, np.float64)
        total = np.zeros(PAD_START, np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            for b in range(6):
                ub, db = u[:, b], d[:, b]
                raw = np.where((ub == 0) | (db == 0), np.float32(0), np.where(ub < db, np.float32(1) - ub / db, db / ub - np.float32(1)))
                assert raw.dtype == np.float32
                rb = raw.astype(np.float64) if b & 1 else -raw.astype(np.float64)
                q = q + rb * n[:, b]
                total = total + n[:, b]
            v = np.where(total > 0, np.abs(q / np.maximum(total, 1) / min_delta / 2.9), 0.0)
        best[r] = v.max() if len(v) else 0.0
        if stats is not None:
            stats.setdefault("block_counts", []).append(counts)
    return best


def scan_centers(speeds, step, n_steps, n_center_steps):
    """SpeedSearch::get_jobs: the centre speeds of a scan pass, in launch order"""
    return [s * math.pow(step, c * (n_steps * 2 + 1)) for s in speeds for c in range(-n_center_steps, n_center_steps + 1)]


def rel_speeds(center, step, n_steps):
    """SpeedSync::get_jobs: (relative speeds, reported speeds) of a centre"""
    rel = [math.pow(step, p) * center / center for p in range(-n_steps, n_steps + 1)]
    return rel, [r * center for r in rel]


def compare_form(n_centers, per, wide, fold):
    """launch_speed_compare's choice restated: "<12>", "<6>fold", "<6>z" or "<1>" """
    ranges = (PAD_START + 255) // 256
    groups6 = (per + 5) // 6
    if wide and 6 < per <= 12 and ranges * n_centers >= 1024:
        return "<12>"
    if ranges * n_centers * groups6 >= 1024 and fold and groups6 > 1:
        return "<6>fold"
    if ranges * n_centers * groups6 >= 1024:
        return "<6>z"
    return "<1>"


# ---- material ------------------------------------------------------------------------------------------------------------------------
N_FRAMES = 60000                         # 44.1 kHz frames of a K13 material: 129 rows at 0.8 need 1.3 x 42 k
GAP_BOTH = (9000, 15000)                 # digital silence in every channel: rows wholly inside at every centre
GAP_RIGHT = (22000, 28000)               # ... in channel 1 (and 2) only
TONE_BIN = 37.3                          # the tone's frequency in bins of a 1024-point transform at 44.1 kHz: between two bins


def noise3(seed, n=N_FRAMES):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


def materials():
    """name -> PCM [60000][3] float32; stereo takes the first two channels, mono the first"""
    n = N_FRAMES
    t = np.arange(n)
    tone = noise3(63) * np.float32(1e-4)
    for c, (df, ph) in enumerate(((0, 0.0), (21.45, 1.0), (-9.7, 2.0))):
        tone[:, c] += (0.9 * np.sin(2 * np.pi * (TONE_BIN + df) * t / 1024 + ph)).astype(np.float32)
    gaps = noise3(64)
    gaps[GAP_BOTH[0]:GAP_BOTH[1]] = 0
    gaps[GAP_RIGHT[0]:GAP_RIGHT[1], 1:] = 0
    return {
        "white": noise3(61),
        "sloped": noise3(62) * np.logspace(0, -3, n, dtype=np.float32)[:, None],
        "tone": tone,
        "pair3": noise3(65) * np.array([1, 1e-3, 1], np.float32),           # the quiet channel rides in the loud one's transform
        "pair6": noise3(66) * np.array([1, 1e-6, 1e-6], np.float32),
        "gaps": gaps,
    }


def k12_inputs(n, C, kind, seed):
    """K12 inputs [n][C] float32: "noise" uniform; "runs" +-1.0 runs of 37 frames with digital silence at both ends; "impulses" one
    impulse per 1000 frames (a wrong tap index moves the output)"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.uniform(-1, 1, (n, C)).astype(np.float32)
    if kind == "runs":
        x = np.repeat(rng.choice(np.array([-1, 1], np.float32), (n // 37 + 1, C)), 37, axis=0)[:n].copy()
        edge = min(n // 4, 300)
        x[:edge] = 0
        x[n - edge:] = 0
        return x
    assert kind == "impulses"
    x = np.zeros((n, C), np.float32)
    x[np.arange(17, n, 1000)] = rng.uniform(0.5, 1, (len(range(17, n, 1000)), C)).astype(np.float32)
    return x
