"""Clip batches straight from signed 16-bit PCM (awm_get_watermark_batch_rates_s16_d, awm_get_watermark_batch_keys_rates_s16_d,
awm_debug_clip_stage_rates_s16_d).

The definition is exact: with f_i = pcm_decode of clip i (float (v) * (1 / 32768), no rounding), the result for clip i is field for field
what the float call returns for f_i at the clip's rate.  So the reference side of every comparison here is the EXISTING float path on
`ctx.pcm_decode` of the same bytes -- never the code under test.  Stage 0 on 16-bit input is held bit for bit, as integers, to the float
stage of every decoded clip ALONE (which tests/test_gpu_get_rate.py and tests/test_gpu_get_rates.py hold to "resample, then copy"); the
pattern lists are compared as whole dicts.  There is no tolerance anywhere in this file.

Shapes: those of tests/test_gpu_get_rates.py -- the tiles are 1024 outputs (generic forms) and 2352 (phase form), so the 44.1 kHz lengths
sit around both, plus lengths of several tiles; the call with 24 clips, one of them 50 s, brings the launcher's rule to several tiles per
workgroup, and so does the group of 64 of the batch test."""
import ctypes as C

import numpy as np
import pytest

from _placement import CANARY, GUARD, Arena, need
from test_get_rates_host import border
from test_gpu_get_rate import ERR_ARG, MATERIALS, PAY1, PAY2, cached, canary_buffers, gpu, launches, material, with_gaps      # noqa: F401 (gpu: the fixture)
from test_gpu_get_rates import LENGTHS, RATES, TILE_P, frames_for

pytestmark = pytest.mark.gpu

FLOAT_STAGE_SCOPES = ("clip_resample_pad_kernel", "clip_stage_mixed_kernel")
S16_OF = {"clip_resample_pad_kernel": "clip_resample_pad_s16_kernel", "clip_stage_mixed_kernel": "clip_stage_mixed_s16_kernel"}
GENERIC, PHASE, COPY = 0, 1, 2


def to_s16(gpu, x):
    """(the clip as 16-bit PCM by the reference's native rule, an int16 tensor shaped like x; its decode, the input of the float reference)"""
    t = gpu.torch
    raw = gpu.ctx.pcm_encode(x.contiguous().view(-1), 16, 0, False, True)
    return raw.view(t.int16).view(x.shape), gpu.ctx.pcm_decode(raw, 16).view(x.shape)


def pairs(gpu, clips):
    both = [to_s16(gpu, c) for c in clips]
    return [b[0] for b in both], [b[1] for b in both]


def channels(clip):
    return 1 if clip.dim() == 1 else clip.shape[1]


def form_launches(gpu):
    out = (C.c_long * 3)()
    gpu.lib.awm_debug_clip_form_launches(out)
    return np.array(list(out))


def stage_check(gpu, clips16, decoded, rates, silent=()):
    """clip_stage_s16 of the group against the float clip_stage of every DECODED clip alone: every value the reference wrote equal as
    integers, every other value of the slice canary or zero, the ranges equal relative to the slice; compared on the device"""
    t = gpu.torch
    ref_buf, got_buf = canary_buffers(gpu, len(clips16), channels(clips16[0]))
    values = ref_buf.shape[1]
    ref_rng = np.zeros((len(clips16), 2), np.int64)
    for i, (c, r) in enumerate(zip(decoded, rates)):
        _, ref_rng[i] = gpu.ctx.clip_stage([c], int(r), out=ref_buf[i:i + 1])              # (slice 0 of its own call: ranges relative to the slice)
    got, got_rng = gpu.ctx.clip_stage_s16(clips16, list(rates), out=got_buf)
    ri, gi = ref_buf.view(t.int32), got.view(t.int32)
    written = ri != CANARY
    assert bool(written.any(dim=1).all()), "the reference wrote nothing into some slice"
    assert not bool(((ri != gi) & written).any()), "a value of the padded slices differs"
    assert bool((written | (gi == CANARY) | (gi == 0)).all()), "a value outside the window is neither canary nor zero"
    for i in range(len(clips16)):
        if tuple(ref_rng[i]) == (-1, 0):
            assert tuple(got_rng[i]) == (-1, 0), (i, got_rng[i])
        else:
            assert tuple(got_rng[i] - i * values) == tuple(ref_rng[i]), (i, ref_rng[i], got_rng[i])
    for i in silent:
        assert tuple(got_rng[i]) == (-1, 0)
    return got


def group_clips(gpu, lengths, rates, ch, kinds, seed):
    return [material(gpu, kinds[i % len(kinds)], seed + i, frames_for(gpu, n44, rates[i]), ch) for i, n44 in enumerate(lengths)]


def with_extremes(x):
    """full scale on both sides (32767 and -32768 after the encode), near both ends and in the middle"""
    x = x.clone()
    flat = x.view(-1)
    n = flat.numel()
    for k, v in ((0, 1.0), (n - 1, -1.0), (n // 2, -1.0), (n // 3, 1.0), (min(n - 1, 5), -1.0), (max(0, n - 7), 1.0)):
        flat[k] = v
    return x


def silent_ends(x):
    """runs of digital silence at both ends"""
    x = x.clone()
    n = x.shape[0]
    x[: n // 6] = 0
    x[n - n // 7:] = 0
    return x


# ---- 1. stage 0, bit for bit ----------------------------------------------------------------------------------------------------------
def test_stage_all_six_rates_every_material(gpu):
    t = gpu.torch
    rates = [RATES[i % 6] for i in range(len(LENGTHS))]
    for kind in MATERIALS:
        clips16, decoded = pairs(gpu, group_clips(gpu, LENGTHS, rates, 2, (kind,), 5100))
        stage_check(gpu, clips16, decoded, rates, silent=range(len(clips16)) if kind == "zero" else ())
    # full scale, silence at both ends, one all-zero clip; the rates shifted against the lengths
    for shift in (1, 4):
        rates = [RATES[(i + shift) % 6] for i in range(len(LENGTHS))]
        clips = group_clips(gpu, LENGTHS, rates, 2, ("noise",), 5200 + 20 * shift)
        clips = [with_extremes(c) if i % 2 else silent_ends(c) for i, c in enumerate(clips)]
        clips[7] = t.zeros_like(clips[7])
        clips16, decoded = pairs(gpu, clips)
        assert int(clips16[1].min()) == -32768 and int(clips16[1].max()) == 32767
        assert not bool(clips16[-2][:100].any()) and not bool(clips16[-2][-100:].any()) and bool(clips16[-2].any())
        stage_check(gpu, clips16, decoded, rates, silent=[7])


ONE_RATE = {48000: ("clip_resample_pad_s16_kernel", PHASE), 32000: ("clip_resample_pad_s16_kernel", GENERIC), 44100: ("clip_pad_s16_kernel", COPY)}


@pytest.mark.parametrize("rate", list(ONE_RATE))
def test_stage_groups_of_one_rate(gpu, rate):
    rates = [rate] * len(LENGTHS)
    clips = group_clips(gpu, LENGTHS, rates, 2, MATERIALS[:3], 5300)
    clips[4] = with_extremes(clips[4])
    clips16, decoded = pairs(gpu, clips)
    stage_check(gpu, clips16, decoded, rates)
    scope, form = ONE_RATE[rate]
    before = form_launches(gpu)
    _, counts = launches(gpu, lambda: gpu.ctx.clip_stage_s16(clips16, rates))
    assert [counts[s] for s in ("clip_pad_s16_kernel", "clip_resample_pad_s16_kernel", "clip_stage_mixed_s16_kernel")] == \
        [int(scope == s) for s in ("clip_pad_s16_kernel", "clip_resample_pad_s16_kernel", "clip_stage_mixed_s16_kernel")], counts
    assert all(counts[s] == 0 for s in FLOAT_STAGE_SCOPES + ("resample_kernel",)), counts
    assert list(form_launches(gpu) - before) == [int(form == f) for f in range(3)]
    # a scalar rate and (44100) the default are the same call
    a, ra = gpu.ctx.clip_stage_s16(clips16[:3], rate)
    b, rb = gpu.ctx.clip_stage_s16(clips16[:3], [rate] * 3)
    assert gpu.torch.equal(a.view(gpu.torch.int32), b.view(gpu.torch.int32)) and np.array_equal(ra, rb)


@pytest.mark.parametrize("ch", [1, 3])
def test_stage_mono_and_three_channels(gpu, ch):
    rates = [RATES[i % 6] for i in range(len(LENGTHS))]
    clips = group_clips(gpu, LENGTHS, rates, ch, MATERIALS, 5400 + ch)
    clips[0], clips[8] = with_extremes(clips[0]), with_extremes(clips[8])
    clips16, decoded = pairs(gpu, clips)
    stage_check(gpu, clips16, decoded, rates, silent=[3, 9])


def shifted(gpu, clip16, values):
    """a copy of the clip that begins `values` int16 values behind a 16-byte boundary"""
    t = gpu.torch
    flat = t.empty(clip16.numel() + 8, dtype=t.int16, device="cuda")
    assert flat.data_ptr() % 16 == 0
    flat[values: values + clip16.numel()].copy_(clip16.reshape(-1))
    out = flat[values: values + clip16.numel()].view(clip16.shape)
    assert out.data_ptr() % 16 == 2 * values and out.is_contiguous()
    return out


def test_stage_one_pointer_only_2_byte_aligned(gpu):
    """the third clip (48 kHz) starts 2 bytes off the 4-byte grid: its group takes the generic taps with scalar loads, bits as before"""
    lengths = (TILE_P + 1, 1025, 2 * TILE_P + 1, 8 * 1024 + 3, 1023, 3 * 44100 + 11)
    rates = (32000, 48000, 48000, 44100, 96000, 48000)
    clips16, decoded = pairs(gpu, group_clips(gpu, lengths, rates, 2, MATERIALS[:3], 5600))
    clips16[2] = shifted(gpu, clips16[2], 1)
    before = form_launches(gpu)
    gpu.ctx.clip_stage_s16(clips16, list(rates))
    assert list(form_launches(gpu) - before) == [1, 0, 1]         # every resampled clip through the generic taps, the 44.1 kHz clip copied
    stage_check(gpu, clips16, decoded, rates)
    # ... and with a 44.1 kHz clip off the grid instead (the copy takes any even address): the 48 kHz clips keep the phase form
    clips16[2] = shifted(gpu, clips16[2], 2)
    clips16[3] = shifted(gpu, clips16[3], 3)
    before = form_launches(gpu)
    got, _ = gpu.ctx.clip_stage_s16(clips16, list(rates))
    assert list(form_launches(gpu) - before) == [1, 1, 1]
    stage_check(gpu, clips16, decoded, rates)
    # the one-rate stage at 48 kHz with one such pointer
    sel = [1, 2, 5]
    clips16[2] = shifted(gpu, clips16[2], 5)
    before = form_launches(gpu)
    gpu.ctx.clip_stage_s16([clips16[i] for i in sel], 48000)
    assert list(form_launches(gpu) - before) == [1, 0, 0]
    stage_check(gpu, [clips16[i] for i in sel], [decoded[i] for i in sel], [48000] * 3)


def test_stage_4_but_not_8_byte_aligned_keeps_the_phase_form(gpu):
    lengths = (TILE_P + 1, 1025, 2 * TILE_P + 1, 8 * 1024 + 3, 1023, 3 * 44100 + 11)
    rates = [48000] * len(lengths)
    clips16, decoded = pairs(gpu, group_clips(gpu, lengths, rates, 2, MATERIALS[:3], 5700))
    clips16 = [shifted(gpu, c, 2 + 4 * (i % 2)) for i, c in enumerate(clips16)]
    assert all(c.data_ptr() % 8 == 4 for c in clips16)
    stage_check(gpu, clips16, decoded, rates)
    before = form_launches(gpu)
    _, counts = launches(gpu, lambda: gpu.ctx.clip_stage_s16(clips16, rates))
    assert counts["clip_resample_pad_s16_kernel"] == 1 and counts["clip_stage_mixed_s16_kernel"] == 0, counts
    assert list(form_launches(gpu) - before) == [0, 1, 0]
    # in a mixed group as well
    mixed_rates = [48000, 32000, 48000, 44100, 48000, 96000]
    clips16, decoded = pairs(gpu, group_clips(gpu, lengths, mixed_rates, 2, MATERIALS[:3], 5750))
    clips16 = [shifted(gpu, c, 2) for c in clips16]
    before = form_launches(gpu)
    _, counts = launches(gpu, lambda: gpu.ctx.clip_stage_s16(clips16, mixed_rates))
    assert counts["clip_stage_mixed_s16_kernel"] == 1 and counts["clip_resample_pad_s16_kernel"] == 0, counts
    assert list(form_launches(gpu) - before) == [1, 1, 1]
    stage_check(gpu, clips16, decoded, mixed_rates)


def test_stage_without_the_phase_form(gpu):
    gpu.lib.awm_debug_set_resample_phase(0)
    try:
        rates = [RATES[i % 6] for i in range(len(LENGTHS))]
        clips16, decoded = pairs(gpu, group_clips(gpu, LENGTHS, rates, 2, MATERIALS, 5800))
        stage_check(gpu, clips16, decoded, rates, silent=[3, 9])
        stage_check(gpu, clips16[1::6], decoded[1::6], [48000, 48000])
    finally:
        gpu.lib.awm_debug_set_resample_phase(1)


def test_stage_under_poison(gpu):
    gpu.lib.awm_debug_set_clip_poison(1)
    try:
        for ch in (2, 1):
            rates = [RATES[(i + 2) % 6] for i in range(len(LENGTHS))]
            clips16, decoded = pairs(gpu, group_clips(gpu, LENGTHS, rates, ch, MATERIALS[:3], 5900 + ch))
            stage_check(gpu, clips16, decoded, rates)
        for rate in (48000, 44100):
            stage_check(gpu, clips16[:4], decoded[:4], [rate] * 4)
    finally:
        gpu.lib.awm_debug_set_clip_poison(0)


@pytest.mark.parametrize("phase", [1, 0], ids=["phase", "generic"])
def test_stage_several_tiles_per_workgroup(gpu, phase):
    """24 clips, the longest 50 s at 32 kHz, the others 0.4 - 49 s at 48 and 44.1 kHz: several tiles per workgroup, shorter clips end inside a
    workgroup's run"""
    gpu.lib.awm_debug_set_resample_phase(phase)
    try:
        secs = [50.0, 0.4, 7.3, 20.1, 49.0, 3.0] * 4
        rates = [32000] + [(48000, 44100)[i % 2] for i in range(1, 24)]
        clips = [material(gpu, MATERIALS[i % 3], 6000 + i, frames_for(gpu, int(s * 44100) + i, rates[i]), 2) for i, s in enumerate(secs)]
        clips16, decoded = pairs(gpu, clips)
        del clips
        stage_check(gpu, clips16, decoded, rates)
    finally:
        gpu.lib.awm_debug_set_resample_phase(1)


# ---- 2. the batch equals the definition -----------------------------------------------------------------------------------------------
def batch_clips(gpu, ch, n_plain, marked_secs, long_clips, var_clip):
    """(16-bit clips, their decodes, rates, indices of the marked ones, their payloads); the watermark is added in float, then encoded"""
    def make():
        rng = np.random.default_rng(31 + ch)
        rates = [RATES[i % 6] for i in range(n_plain)]
        clips = [gpu.noise(7000 + i, int(rng.integers(3 * r, 6 * r)), ch) for i, r in enumerate(rates)]
        clips[2] = with_extremes(clips[2])
        for i, (s, r) in enumerate(long_clips):
            clips.append(gpu.noise(7200 + i, int(s * r) + 13 * i, ch))
            rates.append(r)
        clips.append(gpu.torch.zeros_like(clips[1]))
        rates.append(48000)
        for i, w in enumerate(("inside", "start", "end")):
            r = (32000, 44100, 96000)[i]
            clips.append(with_gaps(gpu, 7220 + i, 4 * r + 7 * i, ch, w))
            rates.append(r)
        if var_clip:
            clips.append(gpu.noise(7230, 5 * 33333, ch))
            rates.append(33333)
        first_marked = len(clips)
        pays = []
        for i, s in enumerate(marked_secs):
            r = RATES[i % 6]
            pays.append(PAY1 if i % 2 else PAY2)
            clips.append(gpu.ctx.add_watermark(None, pays[-1], gpu.noise(7240 + i, int(s * r) + 101 * i, ch), sample_rate=r))
            rates.append(r)
        clips16, decoded = pairs(gpu, clips)
        return clips16, decoded, rates, list(range(first_marked, len(clips))), pays
    return cached(("batch s16", ch, n_plain, tuple(marked_secs), tuple(long_clips), var_clip), make)


def reference(gpu, key, decoded, rates):
    """the float call on the decoded clips; computed once and left unchanged"""
    return cached(("reference s16", key, tuple(rates), tuple(c.data_ptr() for c in decoded)),
                  lambda: gpu.ctx.get_watermark_batch(key, decoded, sample_rate=list(rates)))


def assert_marked(want, marked, pays):
    """the reference itself finds every payload: the comparison is no equality of empty lists"""
    found = [any(p["bits"] == pay for p in want[i]) for i, pay in zip(marked, pays)]
    assert all(found), found


def check_knobs(gpu, call, want):
    for knob in (gpu.lib.awm_debug_set_clip_poison, gpu.lib.awm_debug_set_group_fallback):
        knob(1)
        try:
            assert call() == want
        finally:
            knob(0)


def test_batch_equals_definition_stereo(gpu):
    clips16, decoded, rates, marked, pays = batch_clips(gpu, 2, 58, (40, 41, 42, 43, 44, 45), ((60, 44100), (55, 48000)), True)
    assert 64 + 3 < len(clips16) <= 128 + 3                         # a full group and a remainder beside the two long clips and the VResampler clip
    want = reference(gpu, None, decoded, rates)
    assert_marked(want, marked, pays)
    call = lambda: gpu.ctx.get_watermark_batch_s16(None, clips16, sample_rate=rates)          # noqa: E731
    got, counts = launches(gpu, call)
    assert got == want
    assert counts["clip_stage_mixed_s16_kernel"] == 2 and all(counts[s] == 0 for s in FLOAT_STAGE_SCOPES), counts
    assert counts["resample_kernel"] == 1 and counts["resample_var_kernel"] == 1, counts       # the 48 kHz long clip and the VResampler clip, on their lanes
    before = gpu.lib.awm_debug_alloc_bytes()
    assert call() == want
    assert gpu.lib.awm_debug_alloc_bytes() == before
    check_knobs(gpu, call, want)


def test_batch_equals_definition_mono(gpu):
    clips16, decoded, rates, marked, pays = batch_clips(gpu, 1, 4, (40, 45), (), False)
    assert len(clips16) == 10
    want = reference(gpu, None, decoded, rates)
    assert_marked(want, marked, pays)
    call = lambda: gpu.ctx.get_watermark_batch_s16(None, clips16, sample_rate=rates)          # noqa: E731
    assert call() == want
    check_knobs(gpu, call, want)


def test_key_per_clip(gpu):
    secs = (40, 4, 42, 5, 45, 3.5, 41, 44)
    rates = [(48000, 44100, 32000, 96000)[i % 4] for i in range(len(secs))]
    keys = [gpu.awm.test_key(1 + i % 3) for i in range(len(secs))]
    clips = [gpu.ctx.add_watermark(k, PAY1 if i % 2 else PAY2, gpu.noise(7400 + i, int(s * r) + i, 2), sample_rate=r)
             for i, (s, r, k) in enumerate(zip(secs, rates, keys))]
    clips16, decoded = pairs(gpu, clips)
    want = gpu.ctx.get_watermark_batch_keys(keys, decoded, sample_rate=rates)
    assert_marked(want, [0, 2, 4, 6, 7], [PAY2, PAY2, PAY2, PAY2, PAY1])
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch_keys_s16(keys, clips16, sample_rate=rates))
    assert got == want
    assert counts["clip_stage_mixed_s16_kernel"] == 1 and all(counts[s] == 0 for s in FLOAT_STAGE_SCOPES), counts
    # a wrong key finds nothing where the right one did
    other = gpu.ctx.get_watermark_batch_keys_s16(keys[1:] + keys[:1], clips16, sample_rate=rates)
    assert not any(p["bits"] == PAY2 for p in other[0])


def test_no_rates_is_the_44100_call(gpu):
    clips = [gpu.noise(7500 + i, int(s * 44100) + i, 2) for i, s in enumerate((4, 9, 6.5, 58))]
    clips.append(gpu.ctx.add_watermark(None, PAY1, gpu.noise(7504, 40 * 44100, 2)))
    clips16, decoded = pairs(gpu, clips)
    want = gpu.ctx.get_watermark_batch(None, decoded)
    assert_marked(want, [4], [PAY1])
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch_s16(None, clips16))         # sample_rates NULL
    assert got == want
    assert counts["clip_pad_s16_kernel"] == 1 and counts["clip_stage_mixed_s16_kernel"] == 0 and counts["clip_resample_pad_s16_kernel"] == 0, counts
    assert counts["resample_kernel"] == 0, counts
    assert gpu.ctx.get_watermark_batch_s16(None, clips16, sample_rate=[44100] * 5) == want
    keys = [gpu.awm.test_key(1 + i % 2) for i in range(5)]
    assert gpu.ctx.get_watermark_batch_keys_s16(keys, clips16) == gpu.ctx.get_watermark_batch_keys(keys, decoded)
    # one other rate for the whole call
    assert gpu.ctx.get_watermark_batch_s16(None, clips16[:3], sample_rate=48000) == gpu.ctx.get_watermark_batch(None, decoded[:3], sample_rate=48000)


def test_frames_per_bit_3(gpu):
    gpu.awm.set_params(frames_per_bit=3)
    try:
        rates = [32000, 44100, 48000, 48000]
        clips = [gpu.noise(7600 + i, int(s * r) + i, 2) for i, (s, r) in enumerate(zip((4, 9, 31), rates))]
        clips.append(gpu.ctx.add_watermark(None, PAY1, gpu.noise(7604, 60 * 48000, 2), sample_rate=48000))
        clips16, decoded = pairs(gpu, clips)
        want = gpu.ctx.get_watermark_batch(None, decoded, sample_rate=rates)
        assert_marked(want, [3], [PAY1])
        got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch_s16(None, clips16, sample_rate=rates))
        assert got == want
        assert counts["clip_stage_mixed_s16_kernel"] == 1, counts
        stage_check(gpu, clips16[:3], decoded[:3], rates[:3])
    finally:
        gpu.awm.set_params()


def test_speed_parameter_set(gpu):
    clips = [gpu.noise(7700, 8 * 32000, 2), gpu.ctx.add_watermark(None, PAY2, gpu.noise(7701, 40 * 48000, 2), sample_rate=48000)]
    rates = [32000, 48000]
    clips16, decoded = pairs(gpu, clips)
    gpu.awm.set_speed_params(detect_speed=True)
    try:
        want = gpu.ctx.get_watermark_batch(None, decoded, sample_rate=rates)
        assert_marked(want, [1], [PAY2])
        got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch_s16(None, clips16, sample_rate=rates))
        assert got == want
        assert all(counts[s] == 0 for s in FLOAT_STAGE_SCOPES + tuple(S16_OF.values()) + ("clip_pad_s16_kernel",)), counts
        assert gpu.lib.awm_debug_lane_pcm_bytes(gpu.ctx._h) >= clips[1].numel() * 4              # everything went over the lanes, decoded first
    finally:
        gpu.awm.set_speed_params()


def test_short_long_border(gpu):
    b = border()
    frames = [frames_for(gpu, b - 1, 48000), frames_for(gpu, b, 48000), b - 1, b]
    rates = [48000, 48000, 44100, 44100]
    paths, n44 = gpu.awm.get_batch_rates_plan(frames, rates)
    assert list(paths) == [0, 1, 0, 1] and list(n44) == [b - 1, b, b - 1, b]
    clips16, decoded = pairs(gpu, [gpu.noise(7800 + i, n, 2) for i, n in enumerate(frames)])
    want = gpu.ctx.get_watermark_batch(None, decoded, sample_rate=rates)
    gpu.lib.awm_ctx_trim(gpu.ctx._h)
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch_s16(None, clips16, sample_rate=rates))
    assert got == want
    # the two short clips are one mixed group; of the long ones the one that is not at 44.1 kHz is resampled on its lane
    assert counts["clip_stage_mixed_s16_kernel"] == 1 and counts["resample_kernel"] == 1 and all(counts[s] == 0 for s in FLOAT_STAGE_SCOPES), counts
    # both long clips were decoded into their lanes' workspaces (grow-only buffers round up)
    assert gpu.lib.awm_debug_lane_pcm_bytes(gpu.ctx._h) >= sum(c.numel() for c in clips16[1::2]) * 4


# ---- 3. no float copy, no decode launch -----------------------------------------------------------------------------------------------
def test_short_clips_leave_no_float_copy(gpu):
    lib, ctx = gpu.lib, gpu.ctx
    rates = [RATES[i % 6] for i in range(70)]
    clips = [gpu.noise(7900 + i, 3 * r + 17 * i, 2) for i, r in enumerate(rates)]
    clips16, decoded = pairs(gpu, clips)
    for sel, note in ((slice(None), "mixed"), (slice(1, None, 6), "48 kHz"), (slice(0, None, 6), "44.1 kHz")):
        c16, dec, rs = clips16[sel], decoded[sel], rates[sel]
        want, float_counts = launches(gpu, lambda: ctx.get_watermark_batch(None, dec, sample_rate=rs))
        assert lib.awm_ctx_trim(ctx._h) == 0
        assert lib.awm_debug_lane_pcm_bytes(ctx._h) == 0
        got, counts = launches(gpu, lambda: ctx.get_watermark_batch_s16(None, c16, sample_rate=rs))
        assert got == want, note
        for scope in FLOAT_STAGE_SCOPES:
            assert counts[scope] == 0, (note, counts)
            assert counts[S16_OF[scope]] == float_counts[scope], (note, counts, float_counts)
        assert counts["resample_kernel"] == 0 and counts["resample_var_kernel"] == 0, (note, counts)
        assert counts["clip_pad_s16_kernel"] == (1 if note == "44.1 kHz" else 0), (note, counts)
        assert lib.awm_debug_lane_pcm_bytes(ctx._h) == 0, note
    assert float_counts["clip_stage_mixed_kernel"] == 0 and sum(float_counts[s] for s in FLOAT_STAGE_SCOPES) == 0       # (the last: copies)
    # a long clip does use the workspace, and the trim gives it back
    long16, long_dec = to_s16(gpu, gpu.noise(7990, 60 * 44100, 2))
    assert ctx.get_watermark_batch_s16(None, [long16]) == ctx.get_watermark_batch(None, [long_dec])
    assert lib.awm_debug_lane_pcm_bytes(ctx._h) >= long16.numel() * 4
    assert lib.awm_ctx_trim(ctx._h) == 0 and lib.awm_debug_lane_pcm_bytes(ctx._h) == 0


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    lib, ctx, t = gpu.lib, gpu.ctx, gpu.torch
    x, _ = to_s16(gpu, gpu.noise(8000, 4 * 48000, 2))
    good = (C.c_void_p * 3)(*[x.data_ptr()] * 3)
    frames = (C.c_size_t * 3)(*[x.shape[0] - 1] * 3)
    ok_rates = (C.c_int * 3)(48000, 44100, 32000)
    pats = (gpu.awm.Pattern * 12)()
    keys = bytes(48)

    def refused(ptrs, n_frames, rates, index):
        for fn, key in ((lib.awm_get_watermark_batch_rates_s16_d, bytes(16)), (lib.awm_get_watermark_batch_keys_rates_s16_d, keys)):
            C.memset(pats, 0xA5, C.sizeof(pats))
            n_out = (C.c_int * 3)(-7, -7, -7)
            before = bytes(pats)
            assert fn(ctx._h, key, 3, ptrs, n_frames, 2, rates, 0, 4, pats, n_out) == ERR_ARG
            assert list(n_out) == [-7, -7, -7] and bytes(pats) == before
            assert b"clip %d:" % index in lib.awm_last_error(), lib.awm_last_error()
        rng = np.full((3, 2), -7, np.int64)
        out = t.zeros(16, dtype=t.float32, device="cuda")
        assert lib.awm_debug_clip_stage_rates_s16_d(ctx._h, 3, ptrs, n_frames, 2, rates, C.c_void_p(out.data_ptr()), rng.ctypes.data_as(C.c_void_p)) == ERR_ARG
        assert b"clip %d:" % index in lib.awm_last_error() and (rng == -7).all()
    for at in (0, 2):
        for bad in (0, -1, 1000000):
            rates = [48000, 44100, 32000]
            rates[at] = bad
            refused(good, frames, (C.c_int * 3)(*rates), at)
        odd = [x.data_ptr()] * 3
        odd[at] += 1
        refused((C.c_void_p * 3)(*odd), frames, ok_rates, at)
        refused((C.c_void_p * 3)(*odd), frames, None, at)
        null = [x.data_ptr()] * 3
        null[at] = None
        refused((C.c_void_p * 3)(*null), frames, ok_rates, at)
    # the debug stage: 65 clips, a long clip, a VResampler rate
    rng = np.zeros((65, 2), np.int64)
    out = t.zeros(16, dtype=t.float32, device="cuda")
    ptrs65 = (C.c_void_p * 65)(*[x.data_ptr()] * 65)
    frames65 = (C.c_size_t * 65)(*[1024] * 65)
    rates65 = (C.c_int * 65)(*[(48000, 44100)[i % 2] for i in range(65)])
    assert lib.awm_debug_clip_stage_rates_s16_d(ctx._h, 65, ptrs65, frames65, 2, rates65, C.c_void_p(out.data_ptr()), rng.ctypes.data_as(C.c_void_p)) == ERR_ARG
    long_clip, _ = to_s16(gpu, gpu.noise(8001, 60 * 48000, 2))
    with pytest.raises(gpu.awm.AwmError):
        ctx.clip_stage_s16([x, long_clip], [32000, 48000])
    with pytest.raises(gpu.awm.AwmError):
        ctx.clip_stage_s16([x, x], [48000, 33333])
    with pytest.raises(gpu.awm.AwmError):
        ctx.clip_stage_s16([x, x], [48000, 0])
    # nothing to do
    assert lib.awm_get_watermark_batch_rates_s16_d(ctx._h, bytes(16), 0, None, None, 2, None, 0, 0, None, None) == 0
    assert lib.awm_get_watermark_batch_keys_rates_s16_d(ctx._h, None, 0, None, None, 2, None, 0, 0, None, None) == 0
    assert ctx.get_watermark_batch_s16(None, [], sample_rate=[]) == []
    empty = t.zeros((0, 2), dtype=t.int16, device="cuda")
    got = ctx.get_watermark_batch_s16(None, [empty, x, empty], sample_rate=[48000, 32000, 44100])
    _, dec = to_s16(gpu, gpu.noise(8000, 4 * 48000, 2))
    assert got[0] == [] and got[2] == [] and got[1] == ctx.get_watermark(None, dec, sample_rate=32000)
    # a NULL pointer without frames is an empty clip
    n_out = (C.c_int * 3)(-7, -7, -7)
    null0 = (C.c_void_p * 3)(None, x.data_ptr(), None)
    frames0 = (C.c_size_t * 3)(0, x.shape[0], 0)
    assert lib.awm_get_watermark_batch_rates_s16_d(ctx._h, bytes(16), 3, null0, frames0, 2, ok_rates, 0, 4, pats, n_out) == 0
    assert n_out[0] == 0 and n_out[2] == 0


# ---- 5. placement ---------------------------------------------------------------------------------------------------------------------
def test_placement_of_caller_buffers(gpu):
    """both entry points on guarded caller buffers at 2-, 4- and 16-byte offsets: the guards stay intact, the results are those of the float
    call on the decoded clips, whatever lies beside a clip; the output arrays are written inside their slots only"""
    t, lib, ctx = gpu.torch, gpu.lib, gpu.ctx
    rates = [48000, 32000, 44100, 48000, 44100, 32000, 48000]
    offsets = [2, 4, 2, 4, 16, 6, 16]
    secs = (40, 5, 42, 4, 3, 44, 58)                                # (the last one is long: decoded on a lane)
    keys = [gpu.awm.test_key(1 + i % 2) for i in range(len(secs))]
    marked = [ctx.add_watermark(k, PAY1 if i % 2 else PAY2, gpu.noise(8100 + i, int(s * r) + 13 * i, 2), sample_rate=r)
              for i, (s, r, k) in enumerate(zip(secs, rates, keys))]
    clips16, decoded = pairs(gpu, marked)
    want_keys = ctx.get_watermark_batch_keys(keys, decoded, sample_rate=rates)
    want = ctx.get_watermark_batch(keys[0], decoded, sample_rate=rates)
    assert_marked(want_keys, [0, 2, 5, 6], [PAY2, PAY2, PAY1, PAY2])
    host = [c.cpu().numpy() for c in clips16]
    a = Arena(t, need(*[h.nbytes for h in host]), device="cuda")
    placed = [a.place(h, t.int16, o, name="clip %d" % i) for i, (h, o) in enumerate(zip(host, offsets))]
    assert [p.data_ptr() % 256 for p in placed] == offsets
    assert ctx.get_watermark_batch_s16(keys[0], placed, sample_rate=rates) == want
    a.check()
    assert ctx.get_watermark_batch_keys_s16(keys, placed, sample_rate=rates) == want_keys
    a.check()
    # the output arrays: sentinels beyond what the call may write
    n, slot = len(placed), 8
    ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in placed])
    frames = (C.c_size_t * n)(*[p.shape[0] for p in placed])
    c_rates = (C.c_int * n)(*rates)
    pats = (gpu.awm.Pattern * (n * slot + 2))()
    C.memset(pats, 0xA5, C.sizeof(pats))
    n_out = (C.c_int * (n + 2))(*[-7] * (n + 2))
    assert lib.awm_get_watermark_batch_rates_s16_d(ctx._h, gpu.awm.key_bytes(keys[0]), n, ptrs, frames, 2, c_rates, 0, slot, pats, n_out) == 0
    assert list(n_out)[n:] == [-7, -7] and [n_out[i] for i in range(n)] == [len(w) for w in want]
    size = C.sizeof(gpu.awm.Pattern)
    raw = bytes(pats)
    assert raw[n * slot * size:] == b"\xa5" * (2 * size)
    for i in range(n):
        assert raw[(i * slot + min(n_out[i], slot)) * size: (i + 1) * slot * size] == b"\xa5" * ((slot - min(n_out[i], slot)) * size), i
    # neighbours full of 0x7fff instead of the guards' pattern: nothing beside a clip is read
    for p in placed:
        before, after = a.guard_bytes(p)
        assert before >= GUARD and after >= GUARD
        a.bytes_at(p, -(before // 2 * 2), before // 2 * 2).view(t.int16).fill_(0x7fff)
        a.bytes_at(p, p.numel() * 2, after // 2 * 2).view(t.int16).fill_(0x7fff)
    assert ctx.get_watermark_batch_s16(keys[0], placed, sample_rate=rates) == want
    assert ctx.get_watermark_batch_keys_s16(keys, placed, sample_rate=rates) == want_keys
    small16, small_dec = [p[:3000] for p in placed[:6]], [d[:3000].contiguous() for d in decoded[:6]]
    stage_check(gpu, small16, small_dec, rates[:6])
