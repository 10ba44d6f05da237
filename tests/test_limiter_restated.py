"""The numpy restatement of the limiter (tests/_limiter.py) pinned against the oracle and the compiled reference, and the materials
"dynamics" (D) and "ladder" (L) checked for what they are for.  CPU only.  test_gpu_limiter.py holds every `add` path of the
library to this restatement bit for bit, so it is pinned here first, bit for bit as well:
    add (limiter on) == np_limiter (add (test_no_limiter))
at 44100 Hz and at the rates where the limiter block is another size (block = rate samples), for 1, 2 and 3 channels, on whole
materials and on cuts of them (a partial last block, a last block of one sample, streams shorter than one block).

Why the materials: mutants of the restatement, measured as RMS / max difference to the correct output (the suite's bars for `add`
are 1e-6 RMS and 2e-6 max; `pytest -s` prints the table):

    material                    ramp index + 1         maxima grid + 1        maxima grid - 1
    uniform +-1 noise, 17 s     2.0e-09 / 6.0e-08      0 / 0                  0 / 0                (what the suite had)
    D stereo                    2.5e-07 / 1.4e-05      5.1e-03 / 3.3e-02      3.0e-03 / 1.7e-02
    L stereo                    1.2e-08 / 7.2e-07      2.5e-04 / 1.5e-02      8.8e-04 / 1.6e-02

On full-scale noise every block maximum is about 1.01, the ramps have a slope of 1e-9 per sample and no maximum sits on a block
boundary: a ramp that is one sample off stays 30 x under the bars, and a boundary sample counted in the wrong block changes
nothing at all.  On D and L the shifted grids are far over the bars; the ramp index still is not (D: 1.4e-5 max but 2.5e-7 RMS,
L: under both) -- which is why test_gpu_limiter.py asserts bit-exactness and takes the bars only as its second check."""
import numpy as np
import pytest

import _limiter as lim
import _oracle as orc
import _ref

PAY = "0123456789abcdef0011223344556677"
BS = 44100

# sample rate (== limiter block), channels, frames
SHAPES = [(44100, 2, 5 * BS + 777), (44100, 1, 4 * BS), (44100, 3, 3 * BS + 1), (44100, 2, BS - 5), (44100, 1, BS), (44100, 2, BS + 1),
          (48000, 2, 4 * 48000 + 1), (11025, 1, 4 * 11025), (8000, 2, 5 * 8000 + 9)]


def material(name, ch, block, frames=None):
    x = lim.dynamics(ch, block) if name == "D" else lim.ladder(17, ch, block)
    return x if frames is None else np.ascontiguousarray(x[:frames])


def add_both(mod, x, rate, add=None):
    """(mix, limited) of `mod`: the same add without and with the limiter"""
    add = add or (lambda: mod.add(None, x, x.shape[1], PAY, rate))
    mod.set_params(test_no_limiter=True)
    try:
        mix = add().reshape(x.shape)
    finally:
        mod.set_params()
    return mix, add().reshape(x.shape)


@pytest.mark.parametrize("name", ["D", "L"])
@pytest.mark.parametrize("rate,ch,frames", SHAPES + [(44100, 2, None), (44100, 1, None), (44100, 3, None)])
def test_restatement_equals_the_oracle(name, rate, ch, frames):
    x = material(name, ch, rate, frames)
    mix, limited = add_both(orc, x, rate)
    want, bm = lim.np_limiter(mix, rate)
    assert np.array_equal(lim.bits(limited), lim.bits(want))
    assert len(bm) == -(-len(x) // rate) and bm.min() >= lim.CEILING
    assert np.abs(limited).max() <= np.nextafter(lim.CEILING, np.float32(1))          # limited to the ceiling (one rounding of x * scale)


@pytest.mark.parametrize("name", ["D", "L"])
def test_restatement_equals_the_compiled_reference(name):
    """the same against the unmodified reference sources, where they are built; with one stream that starts inside the grid"""
    if not (_ref.available() and hasattr(_ref.lib(), "ref_add_at")):
        return                                                   # (the oracle pinned it above; nothing more to compare with here)
    for rate, ch, frames in [(44100, 2, None), (44100, 1, 2 * BS + 1), (48000, 2, 3 * 48000 + 1)]:
        x = material(name, ch, rate, frames)
        mix, limited = add_both(_ref, x, rate)
        assert np.array_equal(lim.bits(limited), lim.bits(lim.np_limiter(mix, rate)[0])), (rate, ch, frames)
    x = material(name, 2, BS, 3 * BS + 5)
    zero_frames = BS + 3 * 1024 + 17
    # (the mix of that stream: the plain add of "zeros, then the input" with the zeros cut again.  The reference's own add_stream_watermark
    # is no use for it: with test_no_limiter it still lets the limiter count the skipped zeros, wmadd.cc:513, and then cuts samples.)
    zx = np.concatenate([np.zeros((zero_frames, 2), np.float32), x])
    mix = add_both(_ref, zx, BS)[0][zero_frames:]
    limited = _ref.add_at(None, x, 2, PAY, zero_frames).reshape(x.shape)
    assert np.array_equal(lim.bits(limited), lim.bits(lim.np_limiter(mix, BS, zero_frames=zero_frames)[0]))
    assert not np.array_equal(lim.bits(limited), lim.bits(lim.np_limiter(mix, BS)[0]))       # the offset matters on this material


def test_the_materials_are_what_they_say():
    for ch in (1, 2, 3):
        d = lim.dynamics(ch, BS)
        assert d.shape == (7 * BS + 777, ch)
        want = np.array([0.99, 3, 1.5, 0.99, 0.99, 0.99, 0.995, 2.5], np.float32)
        assert np.array_equal(lim.block_maxima(d, BS), want)
        out, _ = lim.np_limiter(d, BS)
        blk = lambda a, b: slice(b * BS, (b + 1) * BS)
        assert np.array_equal(out[blk(out, 4)], d[blk(d, 4)])                # block 4: the identity entry (1, 0) ...
        assert not np.array_equal(out[blk(out, 3)], d[blk(d, 3)])            # ... and neither neighbour has it
        assert not np.array_equal(out[blk(out, 5)], d[blk(d, 5)])
        l = lim.ladder(17, ch, BS)
        assert l.shape == (17 * BS + 300, ch)
        m = lim.block_maxima(l, BS)
        assert len(m) == 18 and np.all(np.diff(m) > 0.019)                   # rises strictly, block by block
        # the boundaries inside the 128 sample tail of a 1024 sample frame (k = 14, 15) and the wrap behind it (k = 16) are there
        assert [k * BS % 1024 for k in (14, 15, 16)] == [952, 1020, 64]
    # with the watermark in it (the mix that the limiter sees) the maxima keep that shape
    for name, ch in (("D", 2), ("D", 1), ("D", 3), ("L", 2)):
        x = material(name, ch, BS)
        mix, _ = add_both(orc, x, BS)
        m = lim.block_maxima(mix, BS)
        if name == "D":
            assert np.all(m[[0, 3, 4, 5]] == lim.CEILING) and lim.CEILING < m[6] < 1.0 and m[1] > 2.9 and m[2] > 1.4 and m[7] > 2.4
        else:
            assert np.all(np.diff(m) > 0.01)


def mutants(x, block):
    """name -> (output, block maxima) of three wrong limiters"""
    out = {}
    bm = lim.block_maxima(x, block)
    out["ramp index + 1"] = (lim.ramp(x, 0, bm, block, index_offset=1), bm)
    for shift in (1, -1):
        bm_s = lim.block_maxima(x, block, grid_shift=shift)
        out["maxima grid %+d" % shift] = (lim.ramp(x, 0, bm_s, block), bm_s)
    return out


def diff(a, b):
    d = a.astype(np.float64) - b
    return float(np.sqrt((d * d).mean())), float(np.abs(d).max())


def test_mutants_show_on_the_materials():
    """every mutant changes the output on D and on L (so the bit-exact assertion of test_gpu_limiter.py catches it); a shifted grid
    moves a block maximum of L by a whole step of the ladder; on full-scale noise the same mutants are reported, not asserted"""
    for name in ("D", "L"):
        x = material(name, 2, BS)
        mix, _ = add_both(orc, x, BS)
        for what, data in (("input", x), ("mix", mix)):
            good, bm = lim.np_limiter(data, BS)
            for mutant, (out, bm_m) in mutants(data, BS).items():
                r, m = diff(out, good)
                print(f"{name} {what:5s} {mutant:16s} rms {r:.2e} max {m:.2e} largest change of a block maximum {np.abs(bm_m - bm).max():.3f}")
                assert not np.array_equal(lim.bits(out), lim.bits(good)), (name, what, mutant)
                if name == "L" and mutant.startswith("maxima") and what == "input":
                    assert np.abs(bm_m - bm).max() >= 0.02
                    assert np.all(np.abs(bm_m - bm)[1:17] > 0.0199)          # and every block between two boundaries moves by the step
    x = np.random.default_rng(7).uniform(-1, 1, (17 * BS, 2)).astype(np.float32)
    good, _ = lim.np_limiter(x, BS)
    for mutant, (out, _) in mutants(x, BS).items():
        print("uniform +-1 noise %-16s rms %.2e max %.2e" % ((mutant,) + diff(out, good)))


def test_ramp_on_a_span_equals_the_whole():
    """ramp() with first_sample / first_block (what test_gpu_limiter.py expects of add_limit on a span) is the whole stream's limiter
    cut at that place, and table entries under the ceiling count as the ceiling"""
    x = material("D", 2, BS)
    good, bm = lim.np_limiter(x, BS)
    for first, n in ((0, 1), (1, 3), (BS - 1, 2), (BS, BS + 1), (3 * BS + 5, 2 * BS), (len(x) - 1, 1)):
        assert np.array_equal(lim.bits(lim.ramp(x[first:first + n], first, bm, BS)), lim.bits(good[first:first + n]))
        fb = first // BS                                                    # a window of the table that begins at the span's block
        got = lim.ramp(x[first:first + n], first, bm[fb:], BS, first_block=fb)
        if fb == 0 or bm[fb - 1] == lim.CEILING:
            assert np.array_equal(lim.bits(got), lim.bits(good[first:first + n]))
    low = bm.copy()
    low[bm == lim.CEILING] = 0.25
    assert np.array_equal(lim.bits(lim.ramp(x, 0, low, BS)), lim.bits(good))
