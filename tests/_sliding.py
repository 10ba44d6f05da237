"""The refinement's STFT (K4s, csrc/hip/kernels.hip "K4s: refinement STFT by sliding DFT") as a plain float64 transform, and the
inputs that sit on the kernel's special cases.  TEST INFRASTRUCTURE ONLY; plain numpy, no GPU.

ref_db() is what K4s claims to compute, written down without any of its machinery: numpy's float64 rfft of every 1024-sample
window at base + 8 o, weighted in the time domain by the ANALYTIC von Hann window (1/256) (1/2 - 1/2 cos (2 pi n / 1024)) -- the
window K4s applies in the frequency domain --, bins 20..100, then the reference's last float steps (wmcommon.hh:204-218,
syncfinder.cc:594-599): re and im rounded to float32, abs2 = re re + im im in float32, abs2 > 0 ? log2 (abs2) * 3.01029995663981f
: -96, the channels added in float32 as 0 + db0 + db1.  A window whose samples at positions 1..1023 are all zero is a frame of zeros
in the reference (position 0 has weight 0): exactly -96 per channel.  An offset with (idx + 1024) C < first or idx C > last is
skipped: +0 and have = 0 (syncfinder.cc:583-585).  test_sliding_restated.py ties all this to the oracle's sync_fft on the CPU
before test_gpu_sliding_edges.py holds the kernels to it.

THE TOLERANCE is derived per value, not tuned.  K4s computes the transform in double and rounds re and im to float; from there on
it does the reference's float steps.  Against ref_db it may differ by
    - one float32 ulp in re and in im: evaluated by perturbing them and taking the float32 abs2 again (so a denormal abs2 is
      priced as what it is), the largest change of the channel's dB value: the SENSITIVITY term;
    - the logarithm (one ulp: log2f, v_log_f32 per the ISA manual), the multiplication and the two channel additions, one rounding
      each: K ulp32 (|value|).  Every per-channel value here is <= 0 (test_sliding_restated.py asserts it over the case list), so
      the sum's magnitude bounds the parts' and its ulp theirs.
tol = sensitivity + K ulp32 (|value|), K = 4: about 6e-5 dB at -192.  Where a rule fires in every channel (-96, -192, +0) tol is 0.

THE CASES.  One PCM of 48 000 frames per case, a few hundred streams at most; cases() lists them, each with its streams, counts,
table layout and silent ranges.  Every stream's windows end inside the PCM (the kernels take that on trust)."""
import numpy as np

FRAME = 1024
HOP = 8
MIN_BAND, MAX_BAND, NB = 20, 100, 81
ROWS = 60                                # positions of a gathered row: the 30 up and 30 down bands of a sync frame
N_FRAMES = 48000
COUNTS = (65, 64, 63, 49, 48, 33, 32, 31, 17, 16, 15, 2, 1, 0)
K_ULPS = 4
DB_FACTOR = np.float32(3.01029995663981)
WINDOW = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(FRAME) / FRAME)) / 256        # float64


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


def _db64(re, im):
    """the channel's dB value in float64 from float32 re / im through the float32 abs2 (-96 where that is 0)"""
    abs2 = (re * re + im * im).astype(np.float32)
    assert re.dtype == np.float32 and im.dtype == np.float32
    with np.errstate(divide="ignore"):
        return np.where(abs2 > 0, np.log2(abs2.astype(np.float64)), 0.0), abs2


def channel_parts(x, base, count):
    """per channel of x [n][C]: (db [C][count][81] float32, sensitivity [C][count][81] float64, fired [C][count] bool: the
    window carries no weighted non-zero sample)"""
    x = np.asarray(x, np.float32)
    n, C = x.shape
    assert count >= 1 and base >= 0 and base + HOP * (count - 1) + FRAME <= n
    db = np.empty((C, count, NB), np.float32)
    sens = np.zeros((C, count, NB), np.float64)
    fired = np.zeros((C, count), bool)
    for c in range(C):
        seg = x[base:base + HOP * (count - 1) + FRAME, c]
        win = np.lib.stride_tricks.sliding_window_view(seg, FRAME)[::HOP]
        assert win.shape == (count, FRAME)
        fired[c] = ~(win[:, 1:] != 0).any(axis=1)
        spect = np.fft.rfft(win.astype(np.float64) * WINDOW, axis=1)[:, MIN_BAND:MAX_BAND + 1]
        re, im = spect.real.astype(np.float32), spect.imag.astype(np.float32)
        with np.errstate(under="ignore"):
            l2, abs2 = _db64(re, im)
            # wmcommon.hh:204-218: log2f of the float abs2 (the float64 logarithm rounded), one float multiplication
            v = np.where(abs2 > 0, l2.astype(np.float32) * DB_FACTOR, np.float32(-96)).astype(np.float32)
            exact = np.where(abs2 > 0, l2 * float(DB_FACTOR), -96.0)
            ure, uim = np.spacing(np.abs(re)), np.spacing(np.abs(im))
            for sr in (-1, 1):
                for si in (-1, 1):
                    l2p, abs2p = _db64((re + np.float32(sr) * ure).astype(np.float32), (im + np.float32(si) * uim).astype(np.float32))
                    sens[c] = np.maximum(sens[c], np.abs(np.where(abs2p > 0, l2p * float(DB_FACTOR), -96.0) - exact))
        db[c] = np.where(fired[c][:, None], np.float32(-96), v)
        sens[c][fired[c]] = 0
    return db, sens, fired


def ref_db(x, base, count, first=0, last=None):
    """(db [count][81] float32, have [count] int8, tol [count][81] float64) of the stream of `count` windows from `base`"""
    x = np.asarray(x, np.float32)
    C = x.shape[1]
    if last is None:
        last = x.size
    parts, sens, fired = channel_parts(x, base, count)
    total = np.zeros((count, NB), np.float32)
    for c in range(C):
        total = total + parts[c]                                 # 0 + db0 + db1, each a float32 addition
    assert total.dtype == np.float32
    tol = sens.sum(axis=0) + K_ULPS * ulp32(total)
    tol[fired.all(axis=0)] = 0
    idx = base + HOP * np.arange(count, dtype=np.int64)
    skip = ((idx + FRAME) * C < first) | (idx * C > last)
    total[skip] = 0
    tol[skip] = 0
    return total, (~skip).astype(np.int8), tol


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def random_tables(rng, slices, rows_per_plane):
    """(row_perm [slices][rpp] int32, band_pos [slices][rpp][81] uint8): a permutation of the plane's rows per slice, and per row 60
    of the 81 bands one-to-one onto the positions 0..59 (255 for the other 21), as the product's tables are: every position taken"""
    perm = np.stack([rng.permutation(rows_per_plane) for _ in range(slices)]).astype(np.int32)
    pos = np.full((slices, rows_per_plane, NB), 255, np.uint8)
    for s in range(slices):
        for w in range(rows_per_plane):
            pos[s, w, rng.permutation(NB)[:ROWS]] = rng.permutation(ROWS)
    return perm, pos


# ---- material ----------------------------------------------------------------------------------------------------------------------
def noise(seed, n=N_FRAMES):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 2)).astype(np.float32)


# the gaps of digital silence of the "gaps" material: (start, end) in frames
GAP_ALIGNED = (6000, 8000)               # both edges multiples of 8, longer than a whole row (1024 + 8 * 64 = 1536)
GAP_ODD = (12003, 14005)                 # neither edge a multiple of 8
GAP_RIGHT = (20000, 22001)               # in the right channel only
GAP_LONE = (30000, 33000)                # ... with one sample left standing in the left channel
LONE_AT = 31500


def gaps_pcm():
    x = noise(11)
    for a, b in (GAP_ALIGNED, GAP_ODD, GAP_LONE):
        x[a:b] = 0
    x[GAP_RIGHT[0]:GAP_RIGHT[1], 1] = 0
    x[LONE_AT, 0] = 0.25
    return x


def gaps_bases():
    """rows sliding into and out of every gap so that the window runs empty (or has only position 0 left) at the transitions
    0 -> 1, 14 -> 15 .. 16 -> 17, 30 -> 31 .. 32 -> 33, 62 -> 63, 63 -> 64, and first carries a sample again at those offsets;
    rows wholly inside a gap; the lone sample at window position 0 of offset 20 (position 8 at offset 19) and entering at 1023"""
    bases = []
    for a, b in (GAP_ALIGNED, GAP_ODD, GAP_RIGHT, GAP_LONE):
        for o in (1, 15, 16, 17, 31, 32, 33, 63, 64):
            for d in (0, 1, 3):
                bases += [a - HOP * o - d, b - FRAME - HOP * o + d]
    bases += [GAP_ALIGNED[0] + 8, GAP_ALIGNED[0] + 301, GAP_ODD[0] + 5, GAP_RIGHT[0] + 100]
    bases += [LONE_AT - HOP * 20, LONE_AT - HOP * 20 - 1, LONE_AT - 1023 - HOP * 10, LONE_AT - 512 - HOP * 32, LONE_AT - HOP * 64, LONE_AT]
    return bases


LEVEL_TINY = (0, 6000)                   # 1e-15 of full scale
LEVEL_STEP = (8000, 11000, 14000)        # 1e-12, then 1e-16
LEVEL_SLOPE = (16000, 26000)             # 60 dB down
HARD_STEP = 32000                        # full scale, then 1e-6 (not digital silence)


def level_pcm():
    x = noise(12)
    x[LEVEL_TINY[0]:LEVEL_TINY[1]] *= np.float32(1e-15)
    x[LEVEL_STEP[0]:LEVEL_STEP[1]] *= np.float32(1e-12)
    x[LEVEL_STEP[1]:LEVEL_STEP[2]] *= np.float32(1e-16)
    x[LEVEL_SLOPE[0]:LEVEL_SLOPE[1]] *= np.logspace(0, -3, LEVEL_SLOPE[1] - LEVEL_SLOPE[0], dtype=np.float32)[:, None]
    x[HARD_STEP:HARD_STEP + 4000] *= np.float32(1e-6)
    assert (x != 0).all()
    return x


def level_bases():
    bases = [0, 1, 700, 2345, LEVEL_TINY[1] - FRAME - HOP * 64]                                   # every window tiny
    bases += [LEVEL_STEP[1] - FRAME - HOP * o + d for o in (0, 20, 40, 64) for d in (0, 5)]       # 1e-12 sliding out, 1e-16 in
    bases += [LEVEL_STEP[1] - 500, LEVEL_STEP[1] - 77, LEVEL_STEP[1] + 3]
    bases += [LEVEL_SLOPE[0] + 1000 * k + k for k in range(8)]
    bases += [HARD_STEP - FRAME - HOP * o + d for o in (0, 16, 32, 48) for d in (0, 3)]           # the loud part slides out
    bases += [HARD_STEP - HOP * o for o in (64, 40, 20, 1)]                                       # ... and is gone inside the row
    bases += [LEVEL_TINY[1] - 600, LEVEL_STEP[0] - 900]                                           # tiny | full scale | 1e-12
    return bases


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case:
    """one launch: pcm [48000][2] (mono launches take channel 0), bases / counts per stream, rows_per_plane, the tables' slices with
    slice_of [plane] (None: one table, no range_index), and the silent ranges: first / last in FRAMES for all streams, or ranges
    [slice] of (first, last) in frames (first < 0: nothing but silence) looked up through slice_of.  In values the one range is
    [first C, last C) and a slice's [first C + C - 1, last C + C - 1): odd for stereo, where the offset ON the border then falls
    on the other side of the rule than in mono."""

    def __init__(self, name, pcm, bases, counts, rpp, slice_of=None, n_slices=1, first=None, last=None, ranges=None, seed=0):
        self.name, self.pcm, self.rpp = name, pcm, rpp
        self.bases = np.asarray(bases, np.int64)
        self.counts = np.asarray(counts, np.int32)
        assert self.bases.shape == self.counts.shape and self.bases.ndim == 1
        live = self.counts > 0
        assert (self.bases[live] >= 0).all() and (self.bases[live] + HOP * (self.counts[live] - 1) + FRAME <= len(pcm)).all(), name
        assert ((self.counts >= 0) & (self.counts <= 65)).all()
        self.n_planes = -(-len(self.bases) // rpp)
        self.slice_of = None if slice_of is None else np.asarray(slice_of, np.int32)
        assert self.slice_of is None or (len(self.slice_of) == self.n_planes and self.slice_of.max() < n_slices)
        self.n_slices = n_slices
        self.first, self.last, self.ranges = first, last, ranges
        assert ranges is None or (len(ranges) == n_slices and self.slice_of is not None)
        self.perm, self.pos = random_tables(np.random.default_rng(1000 + seed), n_slices, rpp)

    def slice(self, s):
        return 0 if self.slice_of is None else int(self.slice_of[s // self.rpp])

    def slot(self, s):
        return s // self.rpp * self.rpp + int(self.perm[self.slice(s), s % self.rpp])

    def range_values(self, s, C):
        """(first, last) in values for stream s as the kernel is to see them"""
        if self.ranges is not None:
            f, l = self.ranges[self.slice(s)]
            return (-1, -1) if f < 0 else (f * C + (C - 1), l * C + (C - 1))
        f = 0 if self.first is None else self.first * C
        l = len(self.pcm) * C if self.last is None else self.last * C
        return f, l

    def reference(self, C):
        """per stream (db, have, tol, wholly_skipped) or None for count 0; the reference's own ranges: first < 0 is silence everywhere"""
        x = self.pcm[:, :C]
        out = []
        for s, (base, count) in enumerate(zip(self.bases.tolist(), self.counts.tolist())):
            if count == 0:
                out.append(None)
                continue
            f, l = self.range_values(s, C)
            if f < 0:
                f = l = 2 ** 62
            db, have, tol = ref_db(x, base, count, f, l)
            out.append((db, have, tol, not have.any()))
        return out


def _spread(rng, n, count, parity=None):
    hi = N_FRAMES - FRAME - HOP * max(count - 1, 0)
    b = rng.integers(1, hi // 2, n) * 2 + (rng.integers(0, 2, n) if parity is None else parity)
    assert (b <= hi).all()
    return b.tolist()


def end_base(count):
    """the stream's last window ends exactly at the end of the PCM"""
    return N_FRAMES - FRAME - HOP * (max(count, 1) - 1)


def cases():
    rng = np.random.default_rng(77)
    sloped = noise(10) * np.logspace(0, -3, N_FRAMES, dtype=np.float32)[:, None]
    out = []
    # layout: 5 planes of 7 rows and one of 3, a table row of its own per stream, two table slices dealt to the planes out of order
    counts = [COUNTS[i % len(COUNTS)] for i in range(38)]
    bases = [_spread(rng, 1, c, i % 2)[0] for i, c in enumerate(counts)]
    bases[0], bases[1], bases[14] = 0, end_base(counts[1]), end_base(counts[14])
    whole = (0, N_FRAMES)
    out.append(Case("layout", sloped, bases, counts, 7, slice_of=[1, 0, 1, 1, 0, 0], n_slices=2, ranges=[whole, whole], seed=1))
    assert all((p != np.arange(7)).any() for p in out[0].perm) and not np.array_equal(out[0].perm[0], out[0].perm[1])
    # counts x ends: every count at base 0, ending exactly at the end of the PCM, at an odd and at an even base
    counts, bases = [], []
    for c in COUNTS:
        counts += [c] * 4
        bases += [0, end_base(c), _spread(rng, 1, c, 1)[0], _spread(rng, 1, c, 0)[0]]
    out.append(Case("counts", sloped, bases, counts, 3, seed=2))
    # zero rules
    bases = gaps_bases()
    counts = [65] * len(bases)
    for i, c in zip(range(0, len(bases), 9), (64, 49, 33, 48, 63, 32, 17, 31, 16, 15, 2, 1)):
        counts[i] = c
    out.append(Case("gaps", gaps_pcm(), bases, counts, 5, seed=3))
    # level
    bases = level_bases()
    out.append(Case("level", level_pcm(), bases, [65] * len(bases), 4, seed=4))
    # skip rules, one range for all streams: [10000, 30000) frames.  Rows wholly before `first` and wholly behind `last`, rows
    # straddling either (with the offset ON the border: (idx + 1024) C == first and idx C == last are transformed), rows inside
    f, l = 10000, 30000
    bases = [0, 3000, f - FRAME - HOP * 64 - 1, f - FRAME - HOP * 64, f - FRAME - HOP * 30, f - FRAME - HOP * 10 - 3, f - FRAME - 1, f - FRAME,
             f, 20001, l - FRAME, l - HOP * 64, l - HOP * 64 + 1, l - HOP * 30, l - HOP * 10 + 5, l - 1, l, l + 1, l + 8, 40000, end_base(65)]
    counts = [65] * len(bases)
    counts[4], counts[13] = 33, 49
    out.append(Case("skip", sloped, bases, counts, 4, first=f, last=l, seed=5))
    # ... and per slice: slice 0 nothing but silence, slice 1 an odd range, the planes dealt 1 0 1 0 ...
    f, l = 10003, 29999
    bases = [0, f - FRAME - HOP * 64 - 1, f - FRAME - HOP * 40 + 1, f - FRAME - HOP * 16, f - FRAME, 20000, l - HOP * 64 - 1, l - HOP * 33, l - HOP * 16 + 3,
             l, l + 9, end_base(65)]
    bases = [b for b in bases for _ in range(2)]              # rpp = 2 x 12 planes: every base once in a live and once in a silent plane
    bases = bases[0::2] + bases[1::2]
    out.append(Case("skip-slices", sloped, bases, [65] * len(bases), 2, slice_of=[1, 0] * 6, n_slices=2, ranges=[(-1, -1), (f, l)], seed=6))
    return out


def gathered(case, C, n_slots):
    """the reference in the kernel's layout: (want [n_slots][60][65] float32, tol alike, written alike bool: the kernel is to write
    the cell, have_want [n_slots][65] int8 with -1 where nothing is written, loose [n_slots] bool: a wholly skipped row -- its dB cells
    are the kernel's to leave or to fill), from case.reference (C)"""
    want = np.zeros((n_slots, ROWS, 65), np.float32)
    tol = np.zeros((n_slots, ROWS, 65), np.float64)
    written = np.zeros((n_slots, ROWS, 65), bool)
    have = np.full((n_slots, 65), -1, np.int8)
    loose = np.zeros(n_slots, bool)
    seen = set()
    for s, r in enumerate(case.reference(C)):
        slot = case.slot(s)
        assert slot not in seen and slot < n_slots
        seen.add(slot)
        if r is None:
            continue
        db, hv, tl, skipped = r
        count = len(hv)
        have[slot, :count] = hv
        if skipped:
            loose[slot] = True
            continue
        pos = case.pos[case.slice(s), s % case.rpp]
        bands = np.flatnonzero(pos != 255)
        assert sorted(pos[bands].tolist()) == list(range(ROWS))
        want[slot, pos[bands], :count] = db[:, bands].T
        tol[slot, pos[bands], :count] = tl[:, bands].T
        written[slot, :, :count] = True
    return want, tol, written, have, loose
