"""The window of one stream segment at another sample rate (awm_add_segment_plan) against a brute-force model:
every output the mix needs is walked back through the three stages -- up-resampler, K2's three-frame overlap, down-resampler -- with the
window formula of kernels.hh (output m of resampler X reads inputs floor (m step / np) - hl + 1 ... floor (m step / np) + hl of its
stream).  Pure host arithmetic: no GPU."""
import math

import numpy as np
import pytest

import audiowmark_amd as awm

FRAME = 1024
RATES = [48000, 32000, 96000, 22050]


def zita(rate_in, rate_out):
    """(hl, np, step) of zita's fixed-ratio Resampler::setup with hlen 16"""
    g = math.gcd(rate_in, rate_out)
    r = rate_out / rate_in
    hl = 16 if r >= 1 else math.ceil(16 / r)
    return hl, rate_out // g, rate_in // g


def window(m, hl, np_, step):
    b = m * step // np_                        # Python integers: exact at any size
    return b - hl + 1, b + hl


def model(rate, Z, n):
    hd, nd, sd = zita(rate, 44100)
    hu, nu, su = zita(44100, rate)
    # where the watermark begins in front of the segment: the first 44.1 kHz sample whose window sees sample Z, its frame, the frame before
    # it (a frame's spectrum shapes its neighbours), the first output whose window sees that frame.  Found by walking, not by a formula
    q = max(0, (Z - hd) * nd // sd - 2)
    while window(q, hd, nd, sd)[1] < Z:
        q += 1
    w0 = max(0, q // FRAME - 1) * FRAME
    m = max(0, (w0 - hu) * nu // su - 2)
    while window(m, hu, nu, su)[1] < w0:
        m += 1
    mix_first = min(Z, m)
    # the requested outputs mix_first ... Z + n - 1; the window start and end are monotonic in m, so the extremes are at the ends -- plus a
    # sweep over the first and last 4096 outputs that takes nothing for granted
    outs = sorted(set(range(mix_first, min(mix_first + 4096, Z + n))) | set(range(max(mix_first, Z + n - 4096), Z + n)))
    lo = min(max(0, window(k, hu, nu, su)[0]) for k in outs)
    hi = max(window(k, hu, nu, su)[1] for k in outs)
    fa, fb = lo // FRAME, hi // FRAME
    g0, g1 = max(0, fa - 1), fb + 1
    d0, d1 = g0 * FRAME, (g1 + 1) * FRAME - 1
    in_lo = min(window(k, hd, nd, sd)[0] for k in (d0, d0 + 1, d1 - 1, d1))
    in_hi = max(window(k, hd, nd, sd)[1] for k in (d0, d0 + 1, d1 - 1, d1))
    bs = rate
    return dict(mix_first=mix_first, frame_first=fa, frame_last=fb, slice_first=g0, slice_last=g1, down_first=d0, down_last=d1,
                in_first=min(max(in_lo - Z, 0), n - 1), in_last=min(max(in_hi - Z, 0), n - 1), limiter_block=bs,
                first_block=mix_first // bs, n_blocks=(Z + n) // bs + 2 - mix_first // bs,
                down_hl=hd, down_np=nd, down_step=sd, up_hl=hu, up_np=nu, up_step=su)


def cases(rate):
    hd, nd, sd = zita(rate, 44100)
    frame_in = FRAME * sd // nd                # one 44.1 kHz frame in input samples
    ns = [1, 17, 1023, frame_in, rate + 1]
    zs = [0, 1, sd - 1, sd, sd + 1, frame_in - 1, frame_in, frame_in + 1, rate - 1, rate, rate + 1, 2 ** 32 + 12345]
    for n in ns:
        for z in zs + [2 ** 40 - n - 1]:
            yield z, n


@pytest.mark.parametrize("rate", RATES)
def test_plan_matches_the_model(rate):
    for z, n in cases(rate):
        assert awm.add_segment_plan(rate, z, n) == model(rate, z, n), (rate, z, n)


@pytest.mark.parametrize("rate", RATES)
def test_plan_window_is_small_and_encloses_the_segment(rate):
    """what the device path relies on: the slice is the segment's length at 44.1 kHz plus a handful of frames, wherever the segment lies;
    the watermark in front of the segment starts within one limiter block of it"""
    for z, n in cases(rate):
        p = awm.add_segment_plan(rate, z, n)
        assert p["slice_first"] <= p["frame_first"] <= p["frame_last"] < p["slice_last"]
        assert p["slice_last"] - p["slice_first"] + 1 <= n * 44100 // rate // FRAME + 9
        assert 0 <= z - p["mix_first"] < rate and p["first_block"] >= z // rate - 1
        assert p["in_first"] == 0 and p["in_last"] == n - 1          # a few frames of context never end inside the segment


def test_plan_of_an_empty_segment():
    p = awm.add_segment_plan(48000, 12345, 0)
    assert p["n_blocks"] == 0 and p["limiter_block"] == 48000 and (p["down_np"], p["down_step"], p["up_np"], p["up_step"]) == (147, 160, 160, 147)


@pytest.mark.parametrize("rate,z,n", [(44101, 0, 10), (0, 0, 10), (-48000, 0, 10), (48000, 2 ** 40 - 10, 10), (48000, 2 ** 40, 0),
                                      (48000, 5, 2 ** 40), (2000, 0, 10)])
def test_plan_refuses(rate, z, n):
    with pytest.raises(awm.AwmError):
        awm.add_segment_plan(rate, z, n)
