"""The dB of whole frames (K4, K4b: csrc/hip/kernels.hip sync_db_kernel) as a plain float64 transform, the soft bits (K7:
soft_bits_wave_kernel / soft_bits_kernel) restated, and the material that sits on the kernels' special cases.  TEST INFRASTRUCTURE
ONLY; plain numpy, no GPU.  Built on tests/_sliding.py (WINDOW, ulp32, _db64, K_ULPS, the material generators).

ref_db_frames() is what K4 claims to compute: numpy's float64 rfft of the 1024 samples at index + 1024 f, weighted by the analytic von
Hann window, bins 20..100, then the reference's last float steps exactly as _sliding.channel_parts does them (re and im rounded to
float32, the float32 abs2, abs2 > 0 ? log2 (abs2) * 3.01029995663981f : -96), the channels added in float32 as 0 + db0 + db1 + ...
A frame whose samples at positions 1..1023 are all zero is a frame of zeros in the reference: exactly -96 per channel.  A frame with
(idx + 1024) C < first or idx C > last is skipped: +0 and have = 0.  channel_frames() gives the per-channel planes K4b writes.

THE TOLERANCE is derived per value, not tuned.  K4 and K4b transform in float32 (a 512-point complex transform + real_split), so their
re and im carry an ABSOLUTE error of about eps32 ||x w||_2, whatever the bin's own size:
    delta = K_FFT eps32 ||x w||_2   per frame and channel,   eps32 = 2^-23;
re and im are perturbed by +-delta, the four sign pairs, through the float32 abs2; the largest change of the channel's dB value is
the SENSITIVITY term, and where both |re| and |im| are within delta -- abs2 can reach 0 -- the -96 branch counts as well (finite).
    tol = sum over the channels of the sensitivity + K_ULPS ulp32 (|value|),   K_ULPS = 4 as in _sliding
(the logarithm, the multiplication and the channel additions, one rounding each); 0 where a rule fires in every channel.
K_FFT is measured, never against the kernels: test_frames_restated.py takes the largest |X32 - X64| / (eps32 ||x w||_2) of a plain
float32 real transform (scipy.fft.rfft on float32 input, and the reference's own float build where there is one) over every frame of
the case list below and records it as OBSERVED_FFT32; the kernels get twice the larger maximum, for the one more stage of float twiddle
products of the 512-point complex transform + real_split.

soft_bits() is K7 restated from the reference's mix_decode (wmget.cc:67-108): per bit two double accumulators, the terms in the order
frame of the bit, channel, entry; umag += pu[frame]; umag -= double (float32 (pu[prev] + pu[next])) * 0.5; the same for dmag; the
bit is float32 (umag - dmag); neighbours reflected at the block's edges.  With live = (lo, hi) an item whose frame, prev and next all
lie outside [lo, hi] contributes the constants (-96, -192, -96, -192) and reads no plane: the device's rule for blocks of padded
slices.  cells_read() is the mask of every cell some item loads."""
import ctypes
import ctypes.util

import numpy as np

import _sliding as S
from _sliding import DB_FACTOR, FRAME, K_ULPS, MAX_BAND, MIN_BAND, NB, WINDOW, _db64, ulp32  # noqa: F401  (re-exported)

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23
# twice the larger maximum of test_frames_restated.py's OBSERVED_FFT32 (that test asserts the equation)
K_FFT = 2 * 17.8
N_FRAMES = 70000                                 # frames of a K4 material
BLOCK_FRAMES = 2226                              # frames of a block at frames_per_bit 2
BLOCK_PCM_FRAMES = BLOCK_FRAMES * FRAME + 1531   # "2226 x 1024 + a little"
SOFT_BITS = 858


# ---- dB of whole frames --------------------------------------------------------------------------------------------------------------
def frames_of(x, c, index, count):
    return np.asarray(x[index:index + FRAME * count, c]).reshape(count, FRAME)


def spectrum64(frames):
    """(X [count][81] complex128 of the windowed frames, ||x w||_2 [count])"""
    xw = frames.astype(np.float64) * WINDOW
    return np.fft.rfft(xw, axis=1)[:, MIN_BAND:MAX_BAND + 1], np.sqrt((xw * xw).sum(axis=1))


def channel_frames(x, index, count, k_fft=None):
    """per channel of x [n][C]: (db [C][count][81] float32, sensitivity [C][count][81] float64, fired [C][count] bool: the frame
    carries no weighted non-zero sample) of the frames at index + 1024 f"""
    k_fft = K_FFT if k_fft is None else k_fft
    x = np.asarray(x, np.float32)
    n, C = x.shape
    assert count >= 1 and index >= 0 and index + FRAME * count <= n
    db = np.empty((C, count, NB), np.float32)
    sens = np.zeros((C, count, NB), np.float64)
    fired = np.zeros((C, count), bool)
    for c in range(C):
        fr = frames_of(x, c, index, count)
        fired[c] = ~(fr[:, 1:] != 0).any(axis=1)
        spect, norm = spectrum64(fr)
        delta = (k_fft * EPS32 * norm)[:, None]
        re, im = spect.real.astype(np.float32), spect.imag.astype(np.float32)
        with np.errstate(under="ignore"):
            l2, abs2 = _db64(re, im)
            v = np.where(abs2 > 0, l2.astype(np.float32) * DB_FACTOR, np.float32(-96)).astype(np.float32)
            exact = np.where(abs2 > 0, l2 * float(DB_FACTOR), -96.0)
            for sr in (-1, 1):
                for si in (-1, 1):
                    l2p, abs2p = _db64((re.astype(np.float64) + sr * delta).astype(np.float32), (im.astype(np.float64) + si * delta).astype(np.float32))
                    sens[c] = np.maximum(sens[c], np.abs(np.where(abs2p > 0, l2p * float(DB_FACTOR), -96.0) - exact))
            reach0 = (np.abs(re) <= delta) & (np.abs(im) <= delta)              # abs2 can reach 0 under the perturbation: the -96 branch
            sens[c] = np.where(reach0, np.maximum(sens[c], np.abs(-96.0 - exact)), sens[c])
        db[c] = np.where(fired[c][:, None], np.float32(-96), v)
        sens[c][fired[c]] = 0
    return db, sens, fired


def channel_tol(db, sens, fired):
    """the per-channel tolerance of K4b's planes: the channel's own sensitivity + K_ULPS ulp32, 0 where the rule fires"""
    tol = sens + K_ULPS * ulp32(db)
    tol[fired] = 0
    return tol


def ref_db_frames(x, index, count, first=0, last=None):
    """(db [count][81] float32: the channel sum, have [count] int8, tol [count][81] float64) of the frames at index + 1024 f"""
    x = np.asarray(x, np.float32)
    C = x.shape[1]
    if last is None:
        last = x.size
    parts, sens, fired = channel_frames(x, index, count)
    total = np.zeros((count, NB), np.float32)
    for c in range(C):
        total = total + parts[c]                                 # 0 + db0 + db1 + ..., each a float32 addition
    assert total.dtype == np.float32
    tol = sens.sum(axis=0) + K_ULPS * ulp32(total)
    tol[fired.all(axis=0)] = 0
    idx = index + FRAME * np.arange(count, dtype=np.int64)
    skip = ((idx + FRAME) * C < first) | (idx * C > last)
    total[skip] = 0
    tol[skip] = 0
    return total, (~skip).astype(np.int8), tol


def live_frames(base, count, C, first, last):
    """(lo, hi): the frames f of a block at `base` that the skip rule keeps for the value range [first, last) (first < 0: none) --
    by the rule itself, frame by frame.  lo = count, hi = -1 when none is kept"""
    if first < 0:
        return count, -1
    idx = base + FRAME * np.arange(count, dtype=np.int64)
    keep = np.flatnonzero(~(((idx + FRAME) * C < first) | (idx * C > last)))
    if not len(keep):
        return count, -1
    assert (np.diff(keep) == 1).all()
    return int(keep[0]), int(keep[-1])


# ---- soft bits -----------------------------------------------------------------------------------------------------------------------
def mix_entries(key, frames_per_bit=2):
    """_oracle.mix_entries under the oracle's frames_per_bit in force (858 frames_per_bit data frames x 30 entries: frame, up, down)"""
    import _oracle as orc
    if frames_per_bit == 2:
        return orc.mix_entries(key)
    out = np.zeros((SOFT_BITS * frames_per_bit * 30, 3), np.int32)
    n = orc.lib().orc_mix_entries(orc._key(key), orc._p(out))
    assert n == len(out)
    return out


def _items(mix, C, frames_per_bit, block_frames, live):
    """per item of a bit, in summation order: (channel, frame / prev / next / up / down [n_bits], constant [n_bits] bool)"""
    n_bits = len(mix) // 30 // frames_per_bit
    assert len(mix) == n_bits * frames_per_bit * 30
    bits = np.arange(n_bits)
    for i in range(frames_per_bit * C * 30):
        fi, ch, j = i // (C * 30), (i // 30) % C, i % 30
        e = mix[(bits * frames_per_bit + fi) * 30 + j]
        frame, up, down = e[:, 0].astype(np.int64), e[:, 1] - MIN_BAND, e[:, 2] - MIN_BAND
        nxt = np.where(frame + 1 < block_frames, frame + 1, frame - 1)
        prv = np.where(frame - 1 >= 0, frame - 1, frame + 1)
        if live is None:
            const = np.zeros(n_bits, bool)
        else:
            const = (np.maximum(frame, np.maximum(prv, nxt)) < live[0]) | (np.minimum(frame, np.minimum(prv, nxt)) > live[1])
        yield ch, frame, prv, nxt, up, down, const


def soft_bits(planes, mix, frames_per_bit, block_frames, live=None):
    """planes [C][81][>= block_frames] float32 -> [n_bits] float32"""
    planes = np.asarray(planes)
    assert planes.dtype == np.float32 and planes.ndim == 3 and planes.shape[1] == NB and planes.shape[2] >= block_frames
    n_bits = len(mix) // 30 // frames_per_bit
    umag, dmag = np.zeros(n_bits), np.zeros(n_bits)
    c96, c192 = np.float32(-96), np.float32(-96) + np.float32(-96)
    with np.errstate(invalid="ignore"):
        for ch, frame, prv, nxt, up, down, const in _items(mix, planes.shape[0], frames_per_bit, block_frames, live):
            p = planes[ch]
            u0, u1 = p[up, frame], p[up, prv] + p[up, nxt]                      # (float32 additions)
            d0, d1 = p[down, frame], p[down, prv] + p[down, nxt]
            assert u1.dtype == np.float32
            if live is not None:
                u0, u1, d0, d1 = np.where(const, c96, u0), np.where(const, c192, u1), np.where(const, c96, d0), np.where(const, c192, d1)
            umag = umag + u0.astype(np.float64)
            umag = umag - u1.astype(np.float64) * 0.5
            dmag = dmag + d0.astype(np.float64)
            dmag = dmag - d1.astype(np.float64) * 0.5
        return (umag - dmag).astype(np.float32)


def soft_bits_tol(tol_planes, mix, frames_per_bit, block_frames):
    """the per-value tolerances [C][81][frames] carried through the sums with the weights 1 and 1/2 -> [n_bits] float64"""
    n_bits = len(mix) // 30 // frames_per_bit
    total = np.zeros(n_bits)
    for ch, frame, prv, nxt, up, down, _ in _items(mix, tol_planes.shape[0], frames_per_bit, block_frames, None):
        t = tol_planes[ch]
        total += t[up, frame] + 0.5 * (t[up, prv] + t[up, nxt]) + t[down, frame] + 0.5 * (t[down, prv] + t[down, nxt])
    return total


def cells_read(mix, C, frames_per_bit, block_frames, ld, live=None):
    """bool [C][81][ld]: the cells some item of some bit loads"""
    mask = np.zeros((C, NB, ld), bool)
    for ch, frame, prv, nxt, up, down, const in _items(mix, C, frames_per_bit, block_frames, live):
        k = ~const
        for band in (up, down):
            for f in (frame, prv, nxt):
                mask[ch, band[k], f[k]] = True
    return mask


_log2f = None


def db_float_steps(re, im):
    """the reference's db_from_complex on float32 re / im, to the bit: its own log2f (the C library's) and one float multiplication"""
    global _log2f
    if _log2f is None:
        fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").log2f
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
        _log2f = np.frompyfunc(lambda v: fn(v) if v > 0 else 0.0, 1, 1)
    re, im = np.asarray(re, np.float32), np.asarray(im, np.float32)
    with np.errstate(under="ignore"):
        abs2 = (re * re + im * im).astype(np.float32)
    l2 = _log2f(abs2).astype(np.float32)
    return np.where(abs2 > 0, l2 * DB_FACTOR, np.float32(-96)).astype(np.float32)


# ---- material ------------------------------------------------------------------------------------------------------------------------
# gaps of digital silence, whole frames long at any index: (start, end) in frames
GAP_BOTH = (8000, 13000)
GAP_RIGHT = (20000, 25000)               # in the right channel only
GAP_LONE = (30000, 35000)                # ... with one sample left standing in the left channel
LONE_AT = 32000
HARD_STEP = 40000                        # full scale, then 1e-6 (not digital silence)
TONE_BIN = 37.3                          # the strong tone's frequency in bins of the 1024-point transform: between two bins


def _gaps(x):
    for a, b in (GAP_BOTH, GAP_LONE):
        x[a:b] = 0
    x[GAP_RIGHT[0]:GAP_RIGHT[1], 1] = 0
    x[LONE_AT, 0] = 0.25
    return x


def _levels(x):
    x[S.LEVEL_TINY[0]:S.LEVEL_TINY[1]] *= np.float32(1e-15)
    x[S.LEVEL_STEP[0]:S.LEVEL_STEP[1]] *= np.float32(1e-12)
    x[S.LEVEL_STEP[1]:S.LEVEL_STEP[2]] *= np.float32(1e-16)
    x[HARD_STEP:HARD_STEP + 4000] *= np.float32(1e-6)
    assert (x != 0).all()
    return x


def _tone(x):
    """a strong tone over a floor at -80 dB: most bins sit far below the frame's norm"""
    n = np.arange(len(x))
    x *= np.float32(1e-4)
    x[:, 0] += (0.9 * np.sin(2 * np.pi * TONE_BIN * n / FRAME)).astype(np.float32)
    x[:, 1] += (0.9 * np.sin(2 * np.pi * (TONE_BIN + 21.45) * n / FRAME + 1.0)).astype(np.float32)
    return x


def materials():
    """name -> PCM [70000][3] float32; stereo takes the first two channels, mono the first.  The third channel is the right one of
    another noise at a level of its own (-20 dB), with the gaps of the right channel where the material has gaps"""
    n = N_FRAMES
    out = {
        "white": S.noise(21, n),
        "sloped": S.noise(22, n) * np.logspace(0, -3, n, dtype=np.float32)[:, None],
        "gaps": _gaps(S.noise(23, n)),
        "levels": _levels(S.noise(24, n)),
        "tone": _tone(S.noise(25, n)),
        "pair": S.noise(26, n) * np.array([1, 1e-5], np.float32),          # the channels 100 dB apart: a swapped plane cannot hide
    }
    for i, (name, x) in enumerate(out.items()):
        third = S.noise(40 + i, n)[:, 1] * np.float32(0.1)
        third[x[:, 1] == 0] = 0
        out[name] = np.ascontiguousarray(np.concatenate([x, third[:, None]], axis=1))
    return out


def block_pcm():
    """[BLOCK_PCM_FRAMES][3] float32 for whole blocks: white noise that carries every material's feature in a stretch of its own --
    60 dB down the slope over [0.3 M, 0.6 M), the whole-frame gaps (both channels, right only, a lone sample) from 0.7 M, the levels
    from 0.9 M, the tone over its floor over [1.1 M, 1.2 M), and from 1.3 M to the end the right channel 100 dB below the left"""
    n = BLOCK_PCM_FRAMES
    x = S.noise(31, n)
    x[300000:600000] *= np.logspace(0, -3, 300000, dtype=np.float32)[:, None]
    x[700000:700000 + N_FRAMES] = _gaps(x[700000:700000 + N_FRAMES])
    x[900000:900000 + N_FRAMES] = _levels(x[900000:900000 + N_FRAMES])
    x[1100000:1200000] = _tone(x[1100000:1200000])
    x[1300000:, 1] *= np.float32(1e-5)
    third = S.noise(32, n)[:, 1] * np.float32(0.1)
    third[x[:, 1] == 0] = 0
    return np.ascontiguousarray(np.concatenate([x, third[:, None]], axis=1))


def case_frames(index_list=(0, 517)):
    """the case list of the K_FFT measurement and of the CPU checks: for every material the whole frames from each index"""
    for name, x in materials().items():
        for index in index_list:
            yield name, x, index, (len(x) - index) // FRAME
