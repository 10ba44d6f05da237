"""The tile stream at sample rates other than 44.1 kHz, without a GPU: the symbols are exported and declared,
awm_add_stream_rate_plan is held to a brute-force model, and the constructors refuse to run without a context.

The model walks every output m of one full period of the chain back through the stages with the window rule of section 9.3 (output m of
resampler X reads inputs b_X (m) - hl_X + 1 ... b_X (m) + hl_X, b_X (m) = floor (m step_X / np_X)): the last watermark sample the up window
reads, its frame, the frame after it (a frame's signal is complete once the next frame was transformed), that frame's last 44.1 kHz sample,
the last input sample its down window reads.  mix_ahead is the largest distance from m to that sample.  The chain repeats once the 44.1 kHz
side has moved by a multiple of 1024 (frames) and of np_down (the down phases): lcm (1024, np_down) samples there."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import audiowmark_amd as awm
from audiowmark_amd import binding

FRAME = 1024
RATES = [48000, 32000, 96000, 22050, 88200, 176400]
SYMBOLS = ["awm_add_stream_create_rate_at", "awm_add_stream_create_payloads_rate_at", "awm_add_stream_sample_rate", "awm_add_stream_rate_plan",
           "awm_debug_resample_span_d"]


def zita(rate_in, rate_out):
    """(hl, np, step) of zita's fixed-ratio Resampler::setup with hlen 16"""
    g = math.gcd(rate_in, rate_out)
    r = rate_out / rate_in
    hl = 16 if r >= 1 else math.ceil(16 / r)
    return hl, rate_out // g, rate_in // g


def model(rate):
    hd, nd, sd = zita(rate, 44100)
    hu, nu, su = zita(44100, rate)
    period44 = math.lcm(FRAME, nd)
    assert period44 * nu % su == 0 and period44 * sd % nd == 0
    period = period44 * nu // su                              # the same stretch in outputs; also period44 * sd / nd input samples
    m = np.arange(period, dtype=np.int64)
    wl = m * su // nu + hu                                    # last watermark sample the mix of m reads
    q = (wl // FRAME + 2) * FRAME - 1                         # last 44.1 kHz sample of the frame after its frame
    last_in = q * sd // nd + hd                               # last input sample that one reads: down_ahead behind b_down (q)
    mix_ahead = int((last_in - m).max())
    far = m + 977 * period                                    # (it is a period: the same distances anywhere else in the stream)
    assert np.array_equal(((far * su // nu + hu) // FRAME + 2) * FRAME * sd // nd - far, (q + 1) * sd // nd - m)
    limiter_block = rate * 1000 // 1000
    min_tile = max(128 * FRAME, -(-(limiter_block + mix_ahead) // FRAME) * FRAME)
    return dict(limiter_block=limiter_block, down_ahead=hd, mix_ahead=mix_ahead, min_tile=min_tile,
                down_hl=hd, down_np=nd, down_step=sd, up_hl=hu, up_np=nu, up_step=su)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_are_exported_and_declared(name):
    assert getattr(awm.lib, name) is not None
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "awm_hip.h")) as f:
        assert name + " (" in f.read()


@pytest.mark.parametrize("rate", RATES)
def test_plan_matches_the_model(rate):
    assert awm.add_stream_rate_plan(rate) == model(rate)


@pytest.mark.parametrize("rate", RATES)
def test_plan_tables_are_the_segment_plan_s(rate):
    p, s = awm.add_stream_rate_plan(rate), awm.add_segment_plan(rate, 0, 0)
    for k in ("down_hl", "down_np", "down_step", "up_hl", "up_np", "up_step", "limiter_block"):
        assert p[k] == s[k], k


@pytest.mark.parametrize("rate", RATES)
def test_what_the_object_relies_on(rate):
    """the launches end on multiples of np and hold back less than down_step + up_np + 1 samples; min_tile's reasoning needs that to be
    no more than mix_ahead, and a tile to be longer than the lag"""
    p = awm.add_stream_rate_plan(rate)
    assert p["down_step"] + p["up_np"] + 1 <= p["mix_ahead"]
    assert 2 * p["min_tile"] - 2 * p["mix_ahead"] >= 2 * p["limiter_block"]
    assert p["min_tile"] % FRAME == 0 and p["min_tile"] >= 128 * FRAME


def test_the_default_tile_is_the_minimum_at_48_khz():
    assert awm.add_stream_rate_plan(48000)["min_tile"] == 128 * FRAME
    assert 128 * FRAME < awm.add_stream_rate_plan(176400)["min_tile"] <= 256 * FRAME


@pytest.mark.parametrize("rate", [0, -48000, 44101, 2000])
def test_plan_refuses(rate):
    with pytest.raises(awm.AwmError):
        awm.add_stream_rate_plan(rate)
    assert awm.lib.awm_add_stream_rate_plan(rate, None) < 0


def test_constructors_need_a_context():
    hexes = (C.c_char_p * 2)(b"0123456789abcdef0011223344556677", b"f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0")
    h = C.c_void_p()
    calls = {
        "awm_add_stream_create_rate_at": lambda: awm.lib.awm_add_stream_create_rate_at(None, bytes(16), hexes[0], 2, 48000, 128, 0, C.byref(h)),
        "awm_add_stream_create_payloads_rate_at":
            lambda: awm.lib.awm_add_stream_create_payloads_rate_at(None, bytes(16), hexes, 2, 2, 48000, 128, 0, C.byref(h)),
        "awm_add_stream_create_rate_at (44100)": lambda: awm.lib.awm_add_stream_create_rate_at(None, bytes(16), hexes[0], 2, 44100, 128, 0, C.byref(h)),
        "awm_debug_resample_span_d": lambda: awm.lib.awm_debug_resample_span_d(None, None, 0, 0, 0, 0, 2, 48000, 44100, None, None),
    }
    for what, call in calls.items():
        rc = call()
        assert rc < 0, what
        assert b"null context" in awm.lib.awm_last_error(), what
        with pytest.raises(awm.AwmError):
            binding._check(rc, what)
    assert not h.value


def test_null_stream_object():
    assert awm.lib.awm_add_stream_sample_rate(None) == 0
