"""Clip batches with a sample rate per clip (awm_get_watermark_batch_rates_d, awm_get_watermark_batch_keys_rates_d,
awm_debug_clip_stage_rates_d).

The definition is exact: the result for clip i is, field for field, what the 44.1 kHz call returns for `resample (clip i, rate i, 44100)`
-- and for the clip itself where its rate is 44100.  Stage 0 of a group whose clips do not share one rate (K10x) is held bit for bit, as
integers, to the existing one-rate stage of every clip ALONE (which tests/test_gpu_get_rate.py holds to "resample, then copy"); the
pattern lists are compared as whole dicts.  There is no tolerance anywhere in this file.

Shapes: the tiles are 1024 outputs (generic forms) and 2352 (phase form), so the 44.1 kHz lengths sit around both, plus lengths of several
tiles; the stage calls hold at most 12 clips (one tile per workgroup), the call with 24 clips, one of them 50 s, brings the launcher's rule
(tiles of the longest clip x clips / 4096) to several tiles per workgroup, and so do the groups of 64 of the batch test."""
import ctypes as C

import numpy as np
import pytest

from _placement import CANARY, Arena, need
from test_gpu_get_rate import (ERR_ARG, MATERIALS, PAY1, PAY2, cached, canary_buffers, gpu, launches, material, with_gaps)      # noqa: F401 (gpu: the fixture)

pytestmark = pytest.mark.gpu

RATES = (44100, 48000, 32000, 96000, 22050, 88200)
TILE_P = 2352
LENGTHS = (1, 2, 1023, 1024, 1025, TILE_P - 1, TILE_P, TILE_P + 1, 2 * TILE_P + 1, 8 * 1024 + 3, 3 * 44100 + 11, 12 * 44100 + 5)


def frames_for(gpu, n44, rate):
    """the smallest input length at `rate` that gives at least n44 frames at 44.1 kHz (going up not every length exists)"""
    if rate == 44100:
        return n44
    n = max(1, n44 * rate // 44100 - 2)
    while gpu.ctx.resample_frames(n, rate, 44100) < n44:
        n += 1
    return n


def channels(clip):
    return 1 if clip.dim() == 1 else clip.shape[1]


def stage_check(gpu, clips, rates, silent=()):
    """clip_stage of the group with a rate per clip against the one-rate clip_stage of every clip alone: every value the reference wrote
    equal as integers, every other value of the slice canary or zero, the ranges equal relative to the slice; compared on the device.
    Returns the slices under test (a buffer that the next call reuses)."""
    t = gpu.torch
    ref_buf, got_buf = canary_buffers(gpu, len(clips), channels(clips[0]))
    values = ref_buf.shape[1]
    ref_rng = np.zeros((len(clips), 2), np.int64)
    for i, (c, r) in enumerate(zip(clips, rates)):
        _, ref_rng[i] = gpu.ctx.clip_stage([c], int(r), out=ref_buf[i:i + 1])              # (slice 0 of its own call: ranges relative to the slice)
    got, got_rng = gpu.ctx.clip_stage(clips, list(rates), out=got_buf)
    ri, gi = ref_buf.view(t.int32), got.view(t.int32)
    written = ri != CANARY
    assert bool(written.any(dim=1).all()), "the reference wrote nothing into some slice"
    assert not bool(((ri != gi) & written).any()), "a value of the padded slices differs"
    assert bool((written | (gi == CANARY) | (gi == 0)).all()), "a value outside the window is neither canary nor zero"
    for i in range(len(clips)):
        if tuple(ref_rng[i]) == (-1, 0):
            assert tuple(got_rng[i]) == (-1, 0), (i, got_rng[i])
        else:
            assert tuple(got_rng[i] - i * values) == tuple(ref_rng[i]), (i, ref_rng[i], got_rng[i])
    for i in silent:
        assert tuple(got_rng[i]) == (-1, 0)
    return got


def group_clips(gpu, lengths, rates, ch, kinds, seed):
    return [material(gpu, kinds[i % len(kinds)], seed + i, frames_for(gpu, n44, rates[i]), ch) for i, n44 in enumerate(lengths)]


# ---- 1. stage 0, bit for bit ----------------------------------------------------------------------------------------------------------
def test_stage_all_six_rates_every_material(gpu):
    rates = [RATES[i % 6] for i in range(len(LENGTHS))]
    for kind in MATERIALS:
        clips = group_clips(gpu, LENGTHS, rates, 2, (kind,), 1100)
        # (a clip of one or two frames whose first quarter / last fifth is "zero" keeps its samples: n // 4 = n // 5 = 0)
        stage_check(gpu, clips, rates, silent=range(len(clips)) if kind == "zero" else ())
    # the rates shifted against the lengths, mixed material in one group
    for shift in (1, 3, 5):
        rates = [RATES[(i + shift) % 6] for i in range(len(LENGTHS))]
        clips = group_clips(gpu, LENGTHS, rates, 2, MATERIALS, 1200 + 20 * shift)
        stage_check(gpu, clips, rates, silent=[3, 9])


GROUPS = {"48k+44.1k": (48000, 44100), "44.1k+48k": (44100, 48000), "32k+88.2k": (32000, 88200), "96k+22.05k+48k": (96000, 22050, 48000)}


@pytest.mark.parametrize("name", list(GROUPS))
def test_stage_groups_of_few_rates(gpu, name):
    rates = [GROUPS[name][i % len(GROUPS[name])] for i in range(len(LENGTHS))]
    clips = group_clips(gpu, LENGTHS, rates, 2, MATERIALS[:3], 1300)
    stage_check(gpu, clips, rates)
    _, counts = launches(gpu, lambda: gpu.ctx.clip_stage(clips, rates))
    assert counts["clip_stage_mixed_kernel"] == 1 and counts["clip_resample_pad_kernel"] == 0, counts
    # a group that happens to share one rate keeps the one-rate stage
    _, counts = launches(gpu, lambda: gpu.ctx.clip_stage(clips[::len(GROUPS[name])], rates[::len(GROUPS[name])]))
    assert counts["clip_stage_mixed_kernel"] == 0, counts


def test_stage_one_clip_per_rate_and_reversed(gpu):
    t = gpu.torch
    lengths = (TILE_P + 1, 8 * 1024 + 3, 1025, 3 * 44100 + 11, 1023, 2 * TILE_P + 1)
    clips = group_clips(gpu, lengths, RATES, 2, MATERIALS[:3], 1400)
    forward = stage_check(gpu, clips, RATES).clone()
    backward = stage_check(gpu, clips[::-1], RATES[::-1])
    assert t.equal(forward.view(t.int32), backward.flip(0).view(t.int32)), "a clip's slice depends on its place in the group"


@pytest.mark.parametrize("ch", [1, 3])
def test_stage_mono_and_three_channels(gpu, ch):
    rates = [RATES[i % 6] for i in range(len(LENGTHS))]
    clips = group_clips(gpu, LENGTHS, rates, ch, MATERIALS, 1500 + ch)
    stage_check(gpu, clips, rates, silent=[3, 9])


def test_stage_one_pointer_only_4_byte_aligned(gpu):
    """the third clip (48 kHz) starts 4 bytes off the 8-byte grid: its group takes the generic taps, bits as before"""
    lengths = (TILE_P + 1, 1025, 2 * TILE_P + 1, 8 * 1024 + 3, 1023, 3 * 44100 + 11)
    rates = (32000, 48000, 48000, 44100, 96000, 48000)
    clips = group_clips(gpu, lengths, rates, 2, MATERIALS[:3], 1600)
    n = clips[2].shape[0]
    flat = gpu.torch.empty(2 * n + 1, dtype=gpu.torch.float32, device="cuda")
    flat[1:].copy_(clips[2].reshape(-1))
    clips[2] = flat[1:].view(n, 2)
    assert clips[2].data_ptr() % 8 == 4 and clips[2].is_contiguous()
    stage_check(gpu, clips, rates)
    clips[3] = clips[3].clone()                         # ... and with a 44.1 kHz clip off the grid instead (the copy takes any alignment)
    n = clips[3].shape[0]
    flat3 = gpu.torch.empty(2 * n + 1, dtype=gpu.torch.float32, device="cuda")
    flat3[1:].copy_(clips[3].reshape(-1))
    clips[3] = flat3[1:].view(n, 2)
    stage_check(gpu, clips, rates)


def test_stage_without_the_phase_form(gpu):
    gpu.lib.awm_debug_set_resample_phase(0)
    try:
        rates = [RATES[i % 6] for i in range(len(LENGTHS))]
        clips = group_clips(gpu, LENGTHS, rates, 2, MATERIALS, 1700)
        stage_check(gpu, clips, rates, silent=[3, 9])
    finally:
        gpu.lib.awm_debug_set_resample_phase(1)


def test_stage_under_poison(gpu):
    gpu.lib.awm_debug_set_clip_poison(1)
    try:
        for ch in (2, 1):
            rates = [RATES[(i + 2) % 6] for i in range(len(LENGTHS))]
            clips = group_clips(gpu, LENGTHS, rates, ch, MATERIALS[:3], 1800 + ch)
            stage_check(gpu, clips, rates)
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
        clips = [material(gpu, MATERIALS[i % 3], 1900 + i, frames_for(gpu, int(s * 44100) + i, rates[i]), 2) for i, s in enumerate(secs)]
        stage_check(gpu, clips, rates)
    finally:
        gpu.lib.awm_debug_set_resample_phase(1)


# ---- 2. the batch equals the definition -----------------------------------------------------------------------------------------------
def definition(gpu, keys, clips, rates):
    """want[i] = get_watermark (key i, resample (clip i, rate i, 44100)), the clip itself at 44100; computed once and left unchanged"""
    def make():
        want = []
        for k, c, r in zip(keys, clips, rates):
            want.append(gpu.ctx.get_watermark(k, c if r == 44100 else gpu.ctx.resample(c, r, 44100)))
        return want
    return cached(("definition rates", tuple(keys), tuple(rates), tuple(c.data_ptr() for c in clips)), make)


def batch_clips(gpu, ch, n_plain, marked_secs, long_clips, var_clip):
    """(clips, rates, indices of the marked ones, their payloads)"""
    def make():
        rng = np.random.default_rng(17 + ch)
        rates = [RATES[i % 6] for i in range(n_plain)]
        clips = [gpu.noise(2000 + i, int(rng.integers(3 * r, 6 * r)), ch) for i, r in enumerate(rates)]
        for i, (s, r) in enumerate(long_clips):
            clips.append(gpu.noise(2200 + i, int(s * r) + 13 * i, ch))
            rates.append(r)
        clips.append(gpu.torch.zeros_like(clips[1]))
        rates.append(48000)
        for i, w in enumerate(("inside", "start", "end")):
            r = (32000, 44100, 96000)[i]
            clips.append(with_gaps(gpu, 2220 + i, 4 * r + 7 * i, ch, w))
            rates.append(r)
        if var_clip:
            clips.append(gpu.noise(2230, 5 * 33333, ch))
            rates.append(33333)
        first_marked = len(clips)
        pays = []
        for i, s in enumerate(marked_secs):
            r = RATES[i % 6]
            pays.append(PAY1 if i % 2 else PAY2)
            clips.append(gpu.ctx.add_watermark(None, pays[-1], gpu.noise(2240 + i, int(s * r) + 101 * i, ch), sample_rate=r))
            rates.append(r)
        return clips, rates, list(range(first_marked, len(clips))), pays
    return cached(("batch rates", ch, n_plain, tuple(marked_secs), tuple(long_clips), var_clip), make)


def check_knobs(gpu, call, want):
    for knob in (gpu.lib.awm_debug_set_clip_poison, gpu.lib.awm_debug_set_group_fallback):
        knob(1)
        try:
            assert call() == want
        finally:
            knob(0)


def test_batch_equals_definition_stereo(gpu):
    clips, rates, marked, pays = batch_clips(gpu, 2, 80, (21, 23, 25, 27, 29, 30), ((55, 48000), (55, 32000), (60, 44100)), True)
    assert 64 + 4 < len(clips) <= 128 + 4                           # two groups beside the three long clips and the VResampler clip
    want = definition(gpu, [None] * len(clips), clips, rates)
    found = [any(p["bits"] == pay for p in want[i]) for i, pay in zip(marked, pays)]
    print("payloads found by the 44.1 kHz definition, per rate:", dict(zip(RATES, found)))
    assert sum(found) >= 5
    call = lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=rates)          # noqa: E731
    got, counts = launches(gpu, call)
    assert got == want
    assert counts["clip_stage_mixed_kernel"] == 2 and counts["clip_resample_pad_kernel"] == 0, counts
    assert counts["resample_kernel"] == 2 and counts["resample_var_kernel"] == 1, counts
    before = gpu.lib.awm_debug_alloc_bytes()
    assert call() == want
    assert gpu.lib.awm_debug_alloc_bytes() == before
    check_knobs(gpu, call, want)


def test_batch_equals_definition_mono(gpu):
    rates = [(48000, 44100, 32000)[i % 3] for i in range(10)]
    clips = [gpu.noise(2300 + i, int((3 + 0.7 * i) * rates[i]), 1) for i in range(4)]
    clips.append(gpu.torch.zeros_like(clips[1]))
    clips += [with_gaps(gpu, 2310 + i, 4 * rates[5 + i] + 7 * i, 1, w) for i, w in enumerate(("inside", "start", "end"))]
    clips += [gpu.ctx.add_watermark(None, PAY1 if i else PAY2, gpu.noise(2320 + i, s * rates[8 + i] + 101 * i, 1), sample_rate=rates[8 + i])
              for i, s in enumerate((25, 30))]
    assert len(clips) == 10 and len(set(rates)) == 3
    want = definition(gpu, [None] * len(clips), clips, rates)
    call = lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=rates)          # noqa: E731
    assert call() == want
    check_knobs(gpu, call, want)


# ---- 4. a key per clip ----------------------------------------------------------------------------------------------------------------
def test_key_per_clip(gpu):
    secs = (22, 4, 26, 5, 30, 3.5, 24, 28)
    rates = [(48000, 44100, 32000, 96000)[i % 4] for i in range(len(secs))]
    keys = [gpu.awm.test_key(1 + i % 3) for i in range(len(secs))]
    clips = [gpu.ctx.add_watermark(k, PAY1 if i % 2 else PAY2, gpu.noise(2400 + i, int(s * r) + i, 2), sample_rate=r)
             for i, (s, r, k) in enumerate(zip(secs, rates, keys))]
    want = [gpu.ctx.get_watermark(k, c if r == 44100 else gpu.ctx.resample(c, r, 44100)) for k, c, r in zip(keys, clips, rates)]
    assert sum(bool(w) for w in want) >= 3
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch_keys(keys, clips, sample_rate=rates))
    assert got == want
    assert counts["clip_stage_mixed_kernel"] == 1 and counts["clip_resample_pad_kernel"] == 0, counts


# ---- 5. the short / long border per rate ----------------------------------------------------------------------------------------------
def test_short_long_border(gpu):
    border = (gpu.lib.awm_debug_clip_slice_values(1) // (3 * 1024) - 5 + 2) * 1024          # (block frames + 2) 1024
    f48 = [frames_for(gpu, border - 1, 48000), frames_for(gpu, border, 48000)]
    assert [gpu.ctx.resample_frames(n, 48000, 44100) for n in f48] == [border - 1, border]
    hi22 = frames_for(gpu, border, 22050)                         # going up not every length exists: the nearest on either side
    f22 = [hi22 - 1, hi22]
    n22 = [gpu.ctx.resample_frames(n, 22050, 44100) for n in f22]
    assert n22[0] < border <= n22[1]
    frames = f48 + f22 + [border - 1, border]
    rates = [48000, 48000, 22050, 22050, 44100, 44100]
    paths, n44 = gpu.awm.get_batch_rates_plan(frames, rates)
    assert list(paths) == [0, 1, 0, 1, 0, 1] and list(n44) == [border - 1, border] + n22 + [border - 1, border]
    clips = [gpu.noise(2500 + i, n, 2) for i, n in enumerate(frames)]
    want = definition(gpu, [None] * 6, clips, rates)
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=rates))
    assert got == want
    # the three short clips are one mixed group; of the long ones the two that are not at 44.1 kHz are resampled on their lanes
    assert counts["clip_stage_mixed_kernel"] == 1 and counts["clip_resample_pad_kernel"] == 0 and counts["resample_kernel"] == 2, counts


# ---- 6. all rates equal ---------------------------------------------------------------------------------------------------------------
def test_all_rates_equal_is_the_one_rate_call(gpu):
    clips = [gpu.noise(2600 + i, int(s * 48000) + i, 2) for i, s in enumerate((4, 9, 6.5))]
    clips.append(gpu.ctx.add_watermark(None, PAY1, gpu.noise(2604, 27 * 48000, 2), sample_rate=48000))
    one_rate = gpu.ctx.get_watermark_batch(None, clips, sample_rate=48000)
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=[48000] * 4))
    assert got == one_rate
    assert counts["clip_resample_pad_kernel"] == 1 and counts["clip_stage_mixed_kernel"] == 0, counts
    keys = [gpu.awm.test_key(1 + i % 2) for i in range(4)]
    assert gpu.ctx.get_watermark_batch_keys(keys, clips, sample_rate=[48000] * 4) == gpu.ctx.get_watermark_batch_keys(keys, clips, sample_rate=48000)
    plain = gpu.ctx.get_watermark_batch(None, clips)                # the same buffers read as 44.1 kHz material
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=[44100] * 4))
    assert got == plain
    assert counts["clip_resample_pad_kernel"] == 0 and counts["clip_stage_mixed_kernel"] == 0 and counts["resample_kernel"] == 0, counts


# ---- 7. other settings ----------------------------------------------------------------------------------------------------------------
def test_speed_parameter_set(gpu):
    clips = [gpu.noise(2700, 8 * 32000, 2), gpu.ctx.add_watermark(None, PAY2, gpu.noise(2701, 28 * 48000, 2), sample_rate=48000)]
    rates = [32000, 48000]
    gpu.awm.set_speed_params(detect_speed=True)
    try:
        one_by_one = [gpu.ctx.get_watermark(None, c, sample_rate=r) for c, r in zip(clips, rates)]
        got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=rates))
        assert got == one_by_one
        assert counts["clip_stage_mixed_kernel"] == 0 and counts["clip_resample_pad_kernel"] == 0, counts
    finally:
        gpu.awm.set_speed_params()


def test_frames_per_bit_3(gpu):
    gpu.awm.set_params(frames_per_bit=3)
    try:
        rates = [32000, 44100, 48000, 48000]
        clips = [gpu.noise(2800 + i, int(s * r) + i, 2) for i, (s, r) in enumerate(zip((4, 9, 31), rates))]
        clips.append(gpu.ctx.add_watermark(None, PAY1, gpu.noise(2804, 45 * 48000, 2), sample_rate=48000))
        want = [gpu.ctx.get_watermark(None, c if r == 44100 else gpu.ctx.resample(c, r, 44100)) for c, r in zip(clips, rates)]
        got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=rates))
        assert got == want
        assert counts["clip_stage_mixed_kernel"] == 1, counts
        stage_check(gpu, clips[:3], rates[:3])
    finally:
        gpu.awm.set_params()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    lib, ctx = gpu.lib, gpu.ctx
    x = gpu.noise(2900, 4 * 48000, 2)
    ptrs = (C.c_void_p * 3)(*[x.data_ptr()] * 3)
    frames = (C.c_size_t * 3)(*[x.shape[0]] * 3)
    pats = (gpu.awm.Pattern * 12)()
    keys = bytes(48)

    def refused(rates, index):
        for fn, key in ((lib.awm_get_watermark_batch_rates_d, bytes(16)), (lib.awm_get_watermark_batch_keys_rates_d, keys)):
            C.memset(pats, 0xA5, C.sizeof(pats))
            n_out = (C.c_int * 3)(-7, -7, -7)
            before = bytes(pats)
            assert fn(ctx._h, key, 3, ptrs, frames, 2, rates, 0, 4, pats, n_out) == ERR_ARG
            assert list(n_out) == [-7, -7, -7] and bytes(pats) == before
            if index is not None:
                assert b"clip %d:" % index in lib.awm_last_error(), lib.awm_last_error()
    for bad in (0, -1, 1000000):
        refused((C.c_int * 3)(bad, 44100, 32000), 0)
        refused((C.c_int * 3)(48000, 44100, bad), 2)
    refused(None, None)
    # the debug stage: 65 clips, a long clip, a VResampler rate
    rng = np.zeros((65, 2), np.int64)
    ptrs65 = (C.c_void_p * 65)(*[x.data_ptr()] * 65)
    frames65 = (C.c_size_t * 65)(*[1024] * 65)
    rates65 = (C.c_int * 65)(*[(48000, 44100)[i % 2] for i in range(65)])
    assert lib.awm_debug_clip_stage_rates_d(ctx._h, 65, ptrs65, frames65, 2, rates65, C.c_void_p(x.data_ptr()), rng.ctypes.data_as(C.c_void_p)) == ERR_ARG
    long_clip = gpu.noise(2901, 60 * 48000, 2)
    with pytest.raises(gpu.awm.AwmError):
        ctx.clip_stage([x, long_clip], [32000, 48000])
    with pytest.raises(gpu.awm.AwmError):
        ctx.clip_stage([x, x], [48000, 33333])
    with pytest.raises(gpu.awm.AwmError):
        ctx.clip_stage([x, x], [48000, 0])
    # nothing to do
    assert lib.awm_get_watermark_batch_rates_d(ctx._h, bytes(16), 0, None, None, 2, None, 0, 0, None, None) == 0
    assert lib.awm_get_watermark_batch_keys_rates_d(ctx._h, None, 0, None, None, 2, None, 0, 0, None, None) == 0
    assert ctx.get_watermark_batch(None, [], sample_rate=[]) == []
    empty = gpu.torch.zeros((0, 2), dtype=gpu.torch.float32, device="cuda")
    got = ctx.get_watermark_batch(None, [empty, x, empty], sample_rate=[48000, 32000, 44100])
    assert got[0] == [] and got[2] == [] and got[1] == ctx.get_watermark(None, x, sample_rate=32000)


# ---- 10. placement --------------------------------------------------------------------------------------------------------------------
def test_placement_of_caller_buffers(gpu):
    """both entry points on guarded caller buffers, two of them misaligned: the guards stay intact, the results are those on aligned copies"""
    t = gpu.torch
    rates = [48000, 32000, 44100, 48000, 44100, 32000]
    offsets = [0, 4, 8, 4, 0, 8]
    secs = (22, 5, 24, 4, 3, 26)
    keys = [gpu.awm.test_key(1 + i % 2) for i in range(6)]
    marked = [gpu.ctx.add_watermark(k, PAY1 if i % 2 else PAY2, gpu.noise(3000 + i, int(s * r) + 13 * i, 2), sample_rate=r)
              for i, (s, r, k) in enumerate(zip(secs, rates, keys))]
    aligned_keys = gpu.ctx.get_watermark_batch_keys(keys, marked, sample_rate=rates)
    aligned = gpu.ctx.get_watermark_batch(keys[0], marked, sample_rate=rates)
    assert aligned_keys == [gpu.ctx.get_watermark(k, c, sample_rate=r) for k, c, r in zip(keys, marked, rates)]
    assert sum(bool(a) for a in aligned_keys) >= 2
    host = [m.cpu().numpy() for m in marked]
    a = Arena(t, need(*[h.nbytes for h in host]), device="cuda")
    placed = [a.place(h, t.float32, o, name="clip %d" % i) for i, (h, o) in enumerate(zip(host, offsets))]
    assert [p.data_ptr() % 16 for p in placed] == offsets
    assert gpu.ctx.get_watermark_batch(keys[0], placed, sample_rate=rates) == aligned
    a.check()
    assert gpu.ctx.get_watermark_batch_keys(keys, placed, sample_rate=rates) == aligned_keys
    a.check()
