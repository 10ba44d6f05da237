"""tests/_speed.py -- the restatements test_gpu_speed_edges.py holds K12, K13 and K14 to -- tied to the oracle (oracle/awm_oracle.cc:
ZitaVResampler, SpeedSync::prepare_mags, SpeedSync::compare) and, where oracle/_ref was built, to the compiled reference through its
ref_* speed shims, so that the GPU test's yardstick is not its author's opinion.  CPU only.

The table: audiowmark_amd.binding.var_resample_table against zita's formula in numpy's float64, within 1 ulp32 (libm's and numpy's
sines differ by an ulp64 at most, which can move one float32 rounding); row 256 is row 0 moved by one tap, exactly, and its first
tap is 0: the window is 0 at t = hl.  (On x86-64 glibc against numpy 2.2.6 the table is equal to the bit.)

var_resample32 against orc.resample_ratio: with zita's accumulated phase (zita_phases) in place of the exact product, bit for bit
everywhere -- the arithmetic is the oracle's; with the exact product, bit for bit wherever the two phases give the same (window, k,
bf) and within 1e-6 elsewhere.  The share of outputs where they differ, 100 000 outputs per ratio, measured on 2026-10-21 (the test
prints it):
    0.49: 0   1 / 1.01: 0   1 / 0.9764: 0   0.8: 0   7.3: 0   1 / 16: 0   -- asserted < 1 %
    0.3, 3.0: 33.3 %   0.625, 1.25, 2.5: 20 %                             -- printed
The second group are the ratios whose step is a short fraction of 256 (256 / 0.3 = 853 1/3: every third output sits on a whole
frame, where the rounded step's product says phase 0 + m 1e-13 and the accumulated phase says 0 or 255.99999999 of the window
before, bf = float32 (0.99999999) = 1).  By the table's symmetry (row 256 is row 0 one tap on) these are the SAME taps and the outputs
differ by the order of the additions at most (max |difference| 0 at four of them, 2.4e-7 at 3.0); the test asserts that every differing output of these ratios is of this kind.

The round-up of var_phase: see _speed.py; first_round_up() is 3 at ratio 3.0 (output 3, and no other within reach), none at 2.5 and 7.3 and at every ratio <= 2, beyond
2^40 at 5.1, 9.9 and 100, and the restatement's branch gives the window of the exact quotient wherever it fires.

K_FFT512: the error of a plain float32 real transform (scipy.fft.rfft on float32 input) against the float64 transform in units of
eps32 ||x w||_2, the largest over bins 20..100 of every row of every material of _speed.materials() resampled to half rate by the
oracle at the centres 0.8 and 1.25.  OBSERVED_FFT512, measured on 2026-10-21 (x86-64, numpy 2.2.6, scipy 1.15.3's pocketfft), rounded up:
    white 4.48 | sloped 4.14 | tone 13.1 | pair3 3.80 | pair6 4.76 | gaps 4.04
_speed.K_FFT512 is twice the largest.  (The oracle's own transform is evaluated in double and rounded once: it measures nothing
here.  It is held to mags64's tolerance with each channel's own norm instead, below; the largest |oracle - mags64| / tol there is 0.07.)

compare against orc.speed_scan, bit for bit (qualities as uint64, speeds exactly), on orc.speed_mags' matrix of every centre: marked
noise replayed at 1.01, rows 0, 1, 170, 858, 4303 and, at 110 s, 18 900 rows where block 1 swaps and block 2 contributes."""
import math

import numpy as np
import pytest

import _oracle as orc
import _ref
import _speed as SP
from audiowmark_amd import binding

KEY = bytes(range(16))
PAYLOAD = "0123456789abcdef0011223344556677"
GENERIC = (0.49, 1 / 1.01, 1 / 0.9764, 0.8, 7.3, 1 / 16)
SHORT_FRACTION = (0.3, 0.625, 1.25, 2.5, 3.0)                 # 256 / ratio is a multiple of 1 / 3 or 1 / 5
GPU_RATIOS = (0.3, 0.49, 0.625, 1 / 1.01, 1.25, 2.5, 3.0, 7.3, 1 / 16, 0.1, 0.4, 0.5, 0.625)
OBSERVED_FFT512 = {"white": 4.48, "sloped": 4.14, "tone": 13.1, "pair3": 3.80, "pair6": 4.76, "gaps": 4.04}


@pytest.fixture(scope="module")
def cols():
    return SP.key_cols(KEY)


# ---- K12 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", GENERIC + SHORT_FRACTION)
def test_table_matches_the_float64_formula(ratio):
    geo = SP.VarGeometry(ratio)
    tab = binding.var_resample_table(ratio)
    assert tab.shape == (257, geo.hl) and tab.dtype == np.float32
    want = SP.zita_table64(geo).astype(np.float32)
    d = np.abs(tab.astype(np.float64) - want.astype(np.float64))
    assert (d <= np.maximum(SP.ulp32(tab), SP.ulp32(want))).all()
    print("ratio %.4f: hl %d, %d of %d table values differ from numpy's by an ulp32" % (ratio, geo.hl, int((d > 0).sum()), tab.size))
    assert np.array_equal(tab[256, 1:].view(np.uint32), tab[0, :-1].view(np.uint32)) and tab[256, 0] == 0


def test_table_refuses_what_zita_refuses():
    for ratio in (1 / 16.001, 256.5, 0.0, -1.0, float("nan")):
        with pytest.raises(binding.AwmError, match="failed to setup vresampler"):
            binding.var_resample_table(ratio)


@pytest.mark.parametrize("C", (1, 2, 3))
@pytest.mark.parametrize("ratio", GENERIC + SHORT_FRACTION)
def test_var_resample32_against_the_oracle(ratio, C):
    geo = SP.VarGeometry(ratio)
    tab = binding.var_resample_table(ratio)
    n_in = int((100000 if ratio > 0.1 else 20000) / ratio) + C
    x = SP.k12_inputs(n_in, C, "noise", int(ratio * 1000) + C)
    want = orc.resample_ratio(x, C, ratio).reshape(-1, C)
    n_out = SP.resample_frames(n_in, ratio)
    assert len(want) == n_out
    zp = SP.zita_phases(geo, n_out)
    as_zita = SP.var_resample32(x, tab, geo.hl, ratio, n_out, phases=zp)
    assert np.array_equal(as_zita.view(np.uint32), want.view(np.uint32))                   # the arithmetic is the oracle's
    info = {}
    got = SP.var_resample32(x, tab, geo.hl, ratio, n_out, info=info)
    eb, ek, ebf, _ = SP.var_phases(geo, range(n_out))
    same = (zp[0] == eb) & (zp[1] == ek) & (zp[2] == ebf)
    share = 1 - same.mean()
    print("ratio %.4f, %d channels: %d outputs, phases differ for %.4f %%, max |difference| there %.3g" %
          (ratio, C, n_out, 100 * share, np.abs(got[~same] - want[~same]).max() if share else 0))
    assert (info["round_ups"] > 0) == (ratio == 3.0)
    assert np.array_equal(got[same].view(np.uint32), want[same].view(np.uint32))
    assert np.abs(got - want).max() <= 1e-6
    if ratio in GENERIC:
        assert share < 0.01
    else:                                                         # phase 0 (+ a little) of a window against phase 255 + 1 of the one before
        d = ~same

        def at0(b, k, bf):
            return (k[d] == 0) & (bf[d] < 1e-6), b[d]

        def at256(b, k, bf):
            return (k[d] == 255) & (bf[d] > 1 - 1e-6), b[d] + 1
        (z0, zb0), (z1, zb1), (e0, eb0), (e1, eb1) = at0(*zp), at256(*zp), at0(eb, ek, ebf), at256(eb, ek, ebf)
        assert ((z0 | z1) & (e0 | e1)).all() and (np.where(z0, zb0, zb1) == np.where(e0, eb0, eb1)).all()


@pytest.mark.parametrize("ratio", sorted(set(GPU_RATIOS)) + [5.1, 9.9, 100.0])
def test_where_the_phase_rounds_up(ratio):
    geo = SP.VarGeometry(ratio)
    m = SP.first_round_up(geo)
    print("ratio %.4f: shift %d, the first output that rounds up is %s" % (ratio, geo.shift, m))
    if ratio <= 2:
        assert geo.shift <= 53 and m is None                      # the fraction is exact in a double
    elif ratio in (2.5, 7.3):
        assert m is None                                          # an even mantissa never reaches the odd residues
    elif ratio == 3.0:
        assert m == 3                                             # 3 * (256 / 3 rounded down) = 256 - 2^-46 rounds to 256: output 3 alone
    else:
        assert m > 1 << 40                                        # (not a ratio of the GPU test: out of any test's reach)
    if m is not None:
        b, k, bf, fired = SP.var_phase(geo, m)
        assert fired and k == 0 and bf == 0 and b == (m * geo.mant >> geo.shift) + 1 == round(m / ratio)
        assert not SP.var_phase(geo, m - 1)[3] and not SP.var_phase(geo, m + 1)[3]


@pytest.mark.parametrize("kind", ("runs", "impulses"))
def test_var_resample32_on_the_other_inputs(kind):
    """the inputs of the GPU test that are not noise: silence at both ends, +-1.0 runs, lone impulses; short inputs (n_in < 2 hl)"""
    for ratio, n_in in ((0.49, 30000), (2.5, 30000), (0.3, 100), (1 / 16, 300)):
        geo = SP.VarGeometry(ratio)
        x = SP.k12_inputs(n_in, 2, kind, 5)
        want = orc.resample_ratio(x, 2, ratio).reshape(-1, 2)
        n_out = SP.resample_frames(n_in, ratio)
        got = SP.var_resample32(x, binding.var_resample_table(ratio), geo.hl, ratio, n_out, phases=SP.zita_phases(geo, n_out))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ratio, n_in)


# ---- K13 -----------------------------------------------------------------------------------------------------------------------------
def fft32_error(m):
    import scipy.fft
    worst = 0.0
    w32 = SP.WINDOW512.astype(np.float32)
    for c in (0.8, 1.25):
        sub = orc.resample_ratio(m, 3, c / 2).reshape(-1, 3)
        rows = SP.rows_of(len(sub))
        idx = SP.HOP * np.arange(rows)[:, None] + np.arange(SP.N512)[None, :]
        for ch in range(3):
            x64, norm, _ = SP.spectrum512(sub, ch, rows)
            x32 = scipy.fft.rfft(sub[idx, ch] * w32, axis=1)[:, SP.MIN_BAND:SP.MAX_BAND + 1]
            assert x32.dtype == np.complex64                      # (a single precision transform, not a rounded double one)
            ok = norm > 0
            d = np.maximum(np.abs(x32.real - x64.real), np.abs(x32.imag - x64.imag))[ok] / (SP.EPS32 * norm[ok])[:, None]
            worst = max(worst, float(d.max()))
    return worst


def test_k_fft512_is_twice_the_measured_float32_transform_error():
    pytest.importorskip("scipy")
    assert SP.K_FFT512 == 2 * max(OBSERVED_FFT512.values())
    for name, m in SP.materials().items():
        got = fft32_error(m)
        print("%s: OBSERVED_FFT512 %.3f (recorded %.3g)" % (name, got, OBSERVED_FFT512[name]))
        assert got <= OBSERVED_FFT512[name] and got >= 0.5 * OBSERVED_FFT512[name], (name, got)


@pytest.mark.parametrize("C", (1, 2, 3))
@pytest.mark.parametrize("name", list(SP.materials()))
def test_mags64_against_the_oracle(cols, name, C):
    x = np.ascontiguousarray(SP.materials()[name][:, :C])
    worst = 0.0
    for center, rows, loc in ((0.8, 129, 0.37), (1.25, 65, 0.0)):
        seconds = SP.seconds_for_rows(rows, center, extra=77)
        start, n_in, n_out, n_rows = SP.mags_geometry(len(x), loc, center, seconds)
        assert n_rows == rows
        want = orc.speed_mags(KEY, x, C, loc, center, seconds)
        sub = orc.resample_ratio(x[start:], C, center / 2, max_in_seconds=seconds / center).reshape(-1, C)
        assert len(sub) == n_out and want.shape == (rows, 510, 2)
        got, tol = SP.mags64(sub, cols, packed=False)
        exact = tol == 0
        assert np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32))
        if name == "gaps":
            full = exact.all(axis=(1, 2))
            assert full.sum() >= 5 and (got[full] == np.float32(-96 * 30 * C)).all()
            if C > 1:                                             # the right channel alone silent: its -96 C' stands in every value
                assert (~full[:, None, None] & (got < -96 * 30 * (C - 1))).any()
        r = np.abs(got.astype(np.float64) - want)[~exact] / tol[~exact]
        worst = max(worst, float(r.max()))
        if _ref.available():
            ref = _ref.speed_mags(KEY, x, C, loc, center, seconds)
            assert np.array_equal(ref.view(np.uint32), want.view(np.uint32))
    print("%s, %d channels: largest |oracle - mags64| / tol %.3g" % (name, C, worst))
    assert worst <= 1


# ---- K14 -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replayed():
    y = orc.add(KEY, orc.gen_noise(KEY, 146 * 44100 * 2), 2, PAYLOAD)
    return orc.resample_ratio(y, 2, 1 / 1.01)


def scan_restated(mags_of, cols, seconds, step, n_steps, n_center_steps, speeds, stats=None):
    out = []
    for c in SP.scan_centers(speeds, step, n_steps, n_center_steps):
        m = mags_of(c)
        rel, reported = SP.rel_speeds(c, step, n_steps)
        q = SP.compare(m, len(m), rel, 0.01, cols, stats)
        out += [(s if v > 0 else 0.0, v) for s, v in zip(reported, q)]
    out.sort(key=lambda p: p[0])
    return np.array([p[0] for p in out]), np.array([p[1] for p in out])


@pytest.mark.parametrize("rows,step,n_steps,n_center_steps", [(0, 1.0007, 2, 1), (1, 1.02, 1, 1), (170, 1.02, 3, 1), (858, 1.0007, 2, 1),
                                                               (4303, 1.0007, 5, 0), (18900, 1.0007, 1, 0)])
def test_compare_against_the_oracle(cols, replayed, rows, step, n_steps, n_center_steps):
    loc = 0.3
    seconds = {858: 5.0, 4303: 25.0, 18900: 110.0}.get(rows) or SP.seconds_for_rows(rows, 1.01 * math.pow(step, n_center_steps * (2 * n_steps + 1)))
    s, q = orc.speed_scan(KEY, replayed, 2, loc, seconds, step, n_steps, n_center_steps, [1.01])
    stats = {}
    ms, mq = scan_restated(lambda c: orc.speed_mags(KEY, replayed, 2, loc, c, seconds), cols, seconds, step, n_steps, n_center_steps, [1.01], stats)
    assert np.array_equal(ms, s) and np.array_equal(mq.view(np.uint64), q.view(np.uint64))
    counts = np.array(stats["block_counts"])
    print("rows %d: best quality %.4f, contributions per block %s" % (rows, q.max(), counts.sum(axis=0).tolist()))
    if rows == 0:
        assert not q.any() and not s.any()
    if rows >= 170:
        assert q.max() > 1 and (counts[:, 1] > 0).all()                                           # block 1's swap counts
    if rows >= 858:
        assert abs(s[q.argmax()] - 1.01) < 2e-3                                                   # a real peak
    if rows == 18900:
        assert (counts[:, 2] > 0).all()
    if _ref.available() and rows in (170, 858):
        rs, rq = _ref.speed_scan(KEY, replayed, 2, loc, seconds, step, n_steps, n_center_steps, [1.01])
        assert np.array_equal(rs, s) and np.array_equal(rq.view(np.uint64), q.view(np.uint64))


def test_launcher_forms_restated():
    """the cases test_gpu_speed_edges.py steers K14's launcher with (35 state ranges of 256)"""
    assert (SP.PAD_START + 255) // 256 == 35
    assert SP.compare_form(3, 13, 0, 1) == "<1>" and SP.compare_form(29, 5, 0, 1) == "<1>"
    assert SP.compare_form(31, 5, 0, 1) == "<6>z" and SP.compare_form(31, 1, 0, 1) == "<6>z" and SP.compare_form(15, 7, 0, 0) == "<6>z"
    assert SP.compare_form(15, 7, 0, 1) == "<6>fold" and SP.compare_form(11, 13, 0, 1) == "<6>fold" and SP.compare_form(31, 13, 1, 1) == "<6>fold"
    assert SP.compare_form(31, 7, 1, 1) == "<12>" and SP.compare_form(31, 12, 1, 0) == "<12>" and SP.compare_form(31, 6, 1, 1) == "<6>z"
