"""`get` on resident material at sample rates other than 44.1 kHz (awm_get_watermark_rate_d, awm_get_watermark_batch_rate_d,
awm_get_watermark_batch_keys_rate_d).

The definition is exact: the result for a clip is, field for field, what the 44.1 kHz call returns for `resample (clip, rate, 44100)`.
Stage 0 of the grouped path (K10c: the clips resampled straight into their padded slices) is held bit for bit, as integers, to "resample,
then the 44.1 kHz stage", and the pattern lists are compared as whole dicts -- there is no tolerance to choose anywhere in this file.

Shapes: K10c's tiles are 1024 (generic forms) and 2352 (phase form) outputs, so the clip lengths sit around both, plus lengths of several
tiles.  With the launcher's rule (tiles of the longest clip x clips / 4096) the eight clips of a stage call stay at one tile per
workgroup whatever their length below 51 s; the call with 24 clips, one of them 50 s, brings it to 5 (phase form) and 8 (generic form),
and so do the groups of 64 in the batch test."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc
from _placement import CANARY
from test_gpu_parity import pkey

pytestmark = pytest.mark.gpu

PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"
R48 = 48000
ERR_ARG = -3            # AWM_ERR_ARG (include/awm_hip.h)
TILE_P = 2352           # outputs per tile of the phase form
LENGTHS = (1, 2, 1023, 1024, 1025, TILE_P - 1, TILE_P, TILE_P + 1, 2 * TILE_P + 1, 8 * 1024 + 3, 3 * 44100 + 11, 12 * 44100 + 5)
GROUPS = (LENGTHS[:6] + LENGTHS[-2:], LENGTHS[6:])          # at most 8 clips per stage call
MATERIALS = ("noise", "quarter", "fifth", "zero", "first", "last")

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    ctx = awm.Context(0)

    class G:
        pass
    g = G()
    g.torch, g.awm, g.ctx, g.lib = torch, awm, ctx, awm.lib
    g.lib.awm_prof_name.restype = C.c_char_p

    def device_noise(seed, n, ch):
        def make():
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed)
            x = torch.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=torch.float32)
            return (x * 2 - 1).contiguous()
        return cached(("noise", seed, n, ch), make)
    g.noise = device_noise
    yield g
    _CACHE.clear()
    awm.lib.awm_debug_set_clip_poison(0)
    awm.lib.awm_debug_set_group_fallback(0)
    awm.lib.awm_debug_set_resample_phase(1)
    awm.set_speed_params()
    awm.set_params()


def in_frames_for(gpu, n44, rate):
    """the smallest input length at `rate` that resample_frames maps to n44 frames at 44.1 kHz -- going up (32 and 22.05 kHz) not every
    length exists: then the smallest that maps to more"""
    n = max(1, n44 * rate // 44100 - 2)
    while gpu.ctx.resample_frames(n, rate, 44100) < n44:
        n += 1
    return n


def material(gpu, kind, seed, n, ch):
    x = gpu.noise(seed, n, ch).clone()
    if kind == "quarter":
        x[:n // 4] = 0
    elif kind == "fifth":
        x[n - n // 5:] = 0
    elif kind in ("zero", "first", "last"):
        x.zero_()
        if kind != "zero":
            x.view(-1)[0 if kind == "first" else -1] = 0.75
    return x


def canary_buffers(gpu, n_clips, ch):
    """two [n_clips, slice values] float32 buffers full of canaries (allocated once per shape)"""
    t = gpu.torch
    values = gpu.lib.awm_debug_clip_slice_values(ch)
    assert values > 0 and values % (3 * 1024 * ch) == 0
    bufs = cached(("canary", n_clips, values), lambda: [t.empty((n_clips, values), dtype=t.float32, device="cuda") for _ in range(2)])
    for b in bufs:
        b.view(t.int32).fill_(CANARY)
    return bufs


def stage_check(gpu, clips, rate, silent=()):
    """clip_stage at `rate` against resample + clip_stage at 44.1 kHz: every value the 44.1 kHz stage wrote equal as integers, every
    other value of the buffer under test canary or zero, ranges equal; compared on the device"""
    t = gpu.torch
    ch = 1 if clips[0].dim() == 1 else clips[0].shape[1]
    ref_buf, got_buf = canary_buffers(gpu, len(clips), ch)
    ref, ref_rng = gpu.ctx.clip_stage([gpu.ctx.resample(c, rate, 44100) for c in clips], 44100, out=ref_buf)
    got, got_rng = gpu.ctx.clip_stage(clips, rate, out=got_buf)
    ri, gi = ref.view(t.int32), got.view(t.int32)
    written = ri != CANARY
    assert int(written.sum()) > 0
    assert not bool(((ri != gi) & written).any()), "a value of the padded slices differs"
    assert bool((written | (gi == CANARY) | (gi == 0)).all()), "a value outside the window is neither canary nor zero"
    assert np.array_equal(ref_rng, got_rng), (ref_rng, got_rng)
    for i in silent:
        assert tuple(got_rng[i]) == (-1, 0)
    return got_rng


FORMS = [(R48, 2, 1), (R48, 2, 0), (32000, 2, 1), (96000, 2, 1), (22050, 2, 1), (88200, 2, 1), (R48, 1, 1), (R48, 3, 1)]


# ---- 1. stage 0, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,ch,phase", FORMS, ids=[f"{r}-{c}ch" + ("" if p else "-generic") for r, c, p in FORMS])
def test_stage_bits(gpu, rate, ch, phase):
    gpu.lib.awm_debug_set_resample_phase(phase)
    try:
        for gi, group in enumerate(GROUPS):
            frames = [in_frames_for(gpu, n44, rate) for n44 in group]
            for kind in MATERIALS:
                clips = [material(gpu, kind, 100 + 10 * gi + i, n, ch) for i, n in enumerate(frames)]
                # (a clip of one or two frames whose first quarter / last fifth is "zero" keeps its samples: n // 4 = n // 5 = 0)
                stage_check(gpu, clips, rate, silent=range(len(clips)) if kind == "zero" else ())
        # mixed material in one group
        clips = [material(gpu, MATERIALS[i % len(MATERIALS)], 300 + i, n, ch) for i, n in enumerate(in_frames_for(gpu, n44, rate) for n44 in GROUPS[0])]
        rng = stage_check(gpu, clips, rate, silent=[3])
        assert rng[0][0] >= 0 and rng[0][1] > rng[0][0]
    finally:
        gpu.lib.awm_debug_set_resample_phase(1)


@pytest.mark.parametrize("phase", [1, 0], ids=["phase", "generic"])
def test_stage_bits_several_tiles_per_workgroup(gpu, phase):
    """24 clips, the longest 50 s: 5 tiles per workgroup in the phase form, 8 in the generic form; shorter clips end inside a workgroup's run"""
    gpu.lib.awm_debug_set_resample_phase(phase)
    try:
        secs = [50.0, 0.4, 7.3, 20.1, 49.0, 3.0] * 4
        clips = [material(gpu, MATERIALS[i % 3], 400 + i, in_frames_for(gpu, int(s * 44100) + i, R48), 2) for i, s in enumerate(secs)]
        stage_check(gpu, clips, R48)
    finally:
        gpu.lib.awm_debug_set_resample_phase(1)


def test_stage_bits_under_poison(gpu):
    gpu.lib.awm_debug_set_clip_poison(1)
    try:
        for rate, ch in ((R48, 2), (32000, 2), (R48, 1)):
            frames = [in_frames_for(gpu, n44, rate) for n44 in GROUPS[1]]
            clips = [material(gpu, MATERIALS[i % 3], 500 + i, n, ch) for i, n in enumerate(frames)]
            stage_check(gpu, clips, rate)
    finally:
        gpu.lib.awm_debug_set_clip_poison(0)


def test_stage_refusals(gpu):
    x = gpu.noise(1, 5 * R48, 2)
    long_clip = gpu.noise(2, 60 * R48, 2)
    with pytest.raises(gpu.awm.AwmError):
        gpu.ctx.clip_stage([x], 33333)                              # a VResampler rate
    with pytest.raises(gpu.awm.AwmError):
        gpu.ctx.clip_stage([long_clip], R48)                        # not short
    ptrs = (C.c_void_p * 65)(*[x.data_ptr()] * 65)
    frames = (C.c_size_t * 65)(*[1024] * 65)
    rng = np.zeros((65, 2), np.int64)
    assert gpu.lib.awm_debug_clip_stage_d(gpu.ctx._h, 65, ptrs, frames, 2, R48, C.c_void_p(x.data_ptr()), rng.ctypes.data_as(C.c_void_p)) == ERR_ARG


# ---- 2. the batch equals the definition -----------------------------------------------------------------------------------------------
def with_gaps(gpu, seed, n, ch, where):
    x = gpu.noise(seed, n, ch).clone()
    if where == "inside":
        x[n // 3: n // 2] = 0
    elif where == "start":
        x[: n // 4] = 0
    elif where == "end":
        x[n - n // 4:] = 0
    return x


def batch_clips(gpu, ch, n_plain, marked_secs, long_secs):
    """(clips at 48 kHz, indices of the marked ones, their payloads)"""
    def make():
        rng = np.random.default_rng(7 + ch)
        clips = [gpu.noise(600 + i, int(rng.integers(3 * R48, 6 * R48)), ch) for i in range(n_plain)]
        clips += [gpu.noise(700 + i, int(s * R48) + 13 * i, ch) for i, s in enumerate(long_secs)]
        clips.append(gpu.torch.zeros_like(clips[0]))
        clips += [with_gaps(gpu, 720 + i, 4 * R48 + 7 * i, ch, w) for i, w in enumerate(("inside", "start", "end"))]
        first_marked = len(clips)
        pays = []
        for i, s in enumerate(marked_secs):
            pays.append(PAY1 if i % 2 else PAY2)
            clips.append(gpu.ctx.add_watermark(None, pays[-1], gpu.noise(740 + i, int(s * R48) + 101 * i, ch), sample_rate=R48))
        return clips, list(range(first_marked, len(clips))), pays
    return cached(("batch", ch, n_plain, tuple(marked_secs), tuple(long_secs)), make)


def definition(gpu, key, clips, rate=R48):
    """the 44.1 kHz copies (computed once and left unchanged) and get_watermark of each"""
    def make():
        copies = [gpu.ctx.resample(c, rate, 44100) for c in clips]
        return copies, [gpu.ctx.get_watermark(key, y) for y in copies]
    return cached(("definition", key, rate, tuple(c.data_ptr() for c in clips)), make)


def launches(gpu, fn):
    """kernel name -> launches of its profiling scope while fn runs"""
    lib, ctx = gpu.lib, gpu.ctx
    ctx.synchronize()
    lib.awm_prof_enable(ctx._h, 1)
    try:
        lib.awm_prof_reset(ctx._h)
        result = fn()
        ctx.synchronize()
        counts = {}
        for i in range(lib.awm_prof_count()):
            n = C.c_long()
            assert lib.awm_prof_read(ctx._h, i, None, C.byref(n), None) == 0
            counts[lib.awm_prof_name(i).decode()] = n.value
    finally:
        lib.awm_prof_enable(ctx._h, 0)
    return result, counts


def test_batch_equals_definition_stereo(gpu):
    clips, marked, pays = batch_clips(gpu, 2, 57, (21, 23, 25, 27, 29, 30), (12, 21, 30, 50))
    assert 64 < len(clips) <= 128                                   # two groups
    copies, want = definition(gpu, None, clips)
    found = sum(any(p["bits"] == pay for p in want[i]) for i, pay in zip(marked, pays))
    print("payloads found by the 44.1 kHz definition:", found, "of", len(marked))
    assert found >= 5
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=R48))
    assert got == want
    assert gpu.ctx.get_watermark_batch(None, copies) == want
    assert counts["clip_resample_pad_kernel"] == 2 and counts["resample_kernel"] == 0, counts
    before = gpu.lib.awm_debug_alloc_bytes()
    assert gpu.ctx.get_watermark_batch(None, clips, sample_rate=R48) == want
    assert gpu.lib.awm_debug_alloc_bytes() == before
    for knob in (gpu.lib.awm_debug_set_clip_poison, gpu.lib.awm_debug_set_group_fallback):
        knob(1)
        try:
            assert gpu.ctx.get_watermark_batch(None, clips, sample_rate=R48) == want
        finally:
            knob(0)


def test_batch_equals_definition_mono(gpu):
    clips, marked, pays = batch_clips(gpu, 1, 4, (25, 30), ())
    assert len(clips) == 10
    copies, want = definition(gpu, None, clips)
    assert gpu.ctx.get_watermark_batch(None, clips, sample_rate=R48) == want
    assert gpu.ctx.get_watermark_batch(None, copies) == want
    for knob in (gpu.lib.awm_debug_set_clip_poison, gpu.lib.awm_debug_set_group_fallback):
        knob(1)
        try:
            assert gpu.ctx.get_watermark_batch(None, clips, sample_rate=R48) == want
        finally:
            knob(0)


# ---- 3. a key per clip ----------------------------------------------------------------------------------------------------------------
def test_key_per_clip(gpu):
    secs = (22, 4, 26, 5, 30, 3.5, 24, 28)
    keys = [gpu.awm.test_key(1 + i % 3) for i in range(len(secs))]
    clips = [gpu.ctx.add_watermark(k, PAY1 if i % 2 else PAY2, gpu.noise(800 + i, int(s * R48) + i, 2), sample_rate=R48)
             for i, (s, k) in enumerate(zip(secs, keys))]
    copies = [gpu.ctx.resample(c, R48, 44100) for c in clips]
    want = gpu.ctx.get_watermark_batch_keys(keys, copies)
    assert gpu.ctx.get_watermark_batch_keys(keys, clips, sample_rate=R48) == want
    assert want == [gpu.ctx.get_watermark(k, y) for k, y in zip(keys, copies)]
    assert sum(bool(w) for w in want) >= 3


# ---- 4. the short / long border -------------------------------------------------------------------------------------------------------
def test_short_long_border(gpu):
    border = (gpu.awm.lib.awm_debug_clip_slice_values(1) // (3 * 1024) - 5 + 2) * 1024          # (block frames + 2) 1024
    frames = [in_frames_for(gpu, border - 1, R48), in_frames_for(gpu, border, R48), 70 * R48]
    assert [gpu.ctx.resample_frames(n, R48, 44100) for n in frames[:2]] == [border - 1, border]
    clips = [gpu.noise(900 + i, n, 2) for i, n in enumerate(frames)]
    _, want = definition(gpu, None, clips)
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=R48))
    assert got == want
    assert counts["clip_resample_pad_kernel"] == 1 and counts["resample_kernel"] == 2, counts


# ---- 5. one stream --------------------------------------------------------------------------------------------------------------------
def test_one_stream(gpu):
    w = gpu.ctx.add_watermark(None, PAY2, gpu.noise(811, 115 * R48, 2), sample_rate=R48)
    want = gpu.ctx.get_watermark(None, gpu.ctx.resample(w, R48, 44100))
    got = gpu.ctx.get_watermark(None, w, sample_rate=R48)
    assert got == want
    oracle = orc.get(None, orc.resample(w.cpu().numpy(), 2, R48, 44100), 2)
    assert [pkey(p) for p in got] == [pkey(p) for p in oracle]
    assert sum(p["bits"] == PAY2 for p in got) >= 3


# ---- 6. a VResampler rate -------------------------------------------------------------------------------------------------------------
def test_vresampler_rate(gpu):
    rate = 33333
    assert gpu.ctx.resample_frames(1000, rate, 44100) > 0
    clips = [gpu.noise(950 + i, int(s * rate), 2) for i, s in enumerate((5, 14.5, 25))]
    _, want = definition(gpu, None, clips, rate)
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=rate))
    assert got == want
    assert counts["clip_resample_pad_kernel"] == 0 and counts["resample_var_kernel"] == 3, counts
    assert gpu.ctx.get_watermark(None, clips[1], sample_rate=rate) == want[1]


# ---- 7. other settings ----------------------------------------------------------------------------------------------------------------
def test_frames_per_bit_3(gpu):
    gpu.awm.set_params(frames_per_bit=3)
    try:
        clips = [gpu.noise(960 + i, int(s * R48) + i, 2) for i, s in enumerate((4, 9, 31))]
        clips.append(gpu.ctx.add_watermark(None, PAY1, gpu.noise(964, 45 * R48, 2), sample_rate=R48))
        copies = [gpu.ctx.resample(c, R48, 44100) for c in clips]
        want = [gpu.ctx.get_watermark(None, y) for y in copies]
        got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=R48))
        assert got == want
        assert counts["clip_resample_pad_kernel"] == 1, counts
        stage_check(gpu, clips[:2], R48)
    finally:
        gpu.awm.set_params()


def test_speed_parameter_set(gpu):
    clips = [gpu.noise(970, 8 * R48, 2), gpu.ctx.add_watermark(None, PAY2, gpu.noise(971, 28 * R48, 2), sample_rate=R48)]
    gpu.awm.set_speed_params(detect_speed=True)
    try:
        one_by_one = [gpu.ctx.get_watermark(None, c, sample_rate=R48) for c in clips]
        assert one_by_one == [gpu.ctx.get_watermark(None, gpu.ctx.resample(c, R48, 44100)) for c in clips]
        got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_batch(None, clips, sample_rate=R48))
        assert got == one_by_one
        assert counts["clip_resample_pad_kernel"] == 0, counts
    finally:
        gpu.awm.set_speed_params()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    lib, ctx = gpu.lib, gpu.ctx
    x = gpu.noise(980, 4 * R48, 2)
    ptrs = (C.c_void_p * 2)(x.data_ptr(), x.data_ptr())
    frames = (C.c_size_t * 2)(x.shape[0], x.shape[0])
    pats = (gpu.awm.Pattern * 8)()
    keys = bytes(32)
    for rate in (0, -1, 1000000):
        C.memset(pats, 0xA5, C.sizeof(pats))
        n_out = (C.c_int * 2)(-7, -7)
        before = bytes(pats)
        assert lib.awm_get_watermark_rate_d(ctx._h, bytes(16), C.c_void_p(x.data_ptr()), x.shape[0], 2, rate, 8, pats) == ERR_ARG
        assert b"not implemented" in lib.awm_last_error()
        assert lib.awm_get_watermark_batch_rate_d(ctx._h, bytes(16), 2, ptrs, frames, 2, rate, 0, 4, pats, n_out) == ERR_ARG
        assert b"not implemented" in lib.awm_last_error()
        assert lib.awm_get_watermark_batch_keys_rate_d(ctx._h, keys, 2, ptrs, frames, 2, rate, 0, 4, pats, n_out) == ERR_ARG
        assert list(n_out) == [-7, -7] and bytes(pats) == before
        assert ctx.resample_frames(1000, rate, 44100) == 0
    y = gpu.noise(981, 6 * 44100, 2)
    n_a, n_b = (C.c_int * 1)(), (C.c_int * 1)()
    one = (C.c_void_p * 1)(y.data_ptr())
    n = (C.c_size_t * 1)(y.shape[0])
    pa, pb = (gpu.awm.Pattern * 8)(), (gpu.awm.Pattern * 8)()
    assert lib.awm_get_watermark_batch_rate_d(ctx._h, bytes(16), 1, one, n, 2, 44100, 0, 8, pa, n_a) == 0
    assert lib.awm_get_watermark_batch_d(ctx._h, bytes(16), 1, one, n, 2, 0, 8, pb, n_b) == 0
    assert n_a[0] == n_b[0] and bytes(pa)[: C.sizeof(gpu.awm.Pattern) * min(8, n_a[0])] == bytes(pb)[: C.sizeof(gpu.awm.Pattern) * min(8, n_b[0])]
    assert lib.awm_get_watermark_rate_d(ctx._h, bytes(16), C.c_void_p(y.data_ptr()), y.shape[0], 2, 44100, 8, pa) == len(ctx.get_watermark(None, y))
    assert ctx.get_watermark_batch(None, [], sample_rate=R48) == []
    assert ctx.get_watermark_batch_keys([], [], sample_rate=R48) == []
    assert lib.awm_get_watermark_batch_rate_d(ctx._h, bytes(16), 0, None, None, 2, R48, 0, 0, None, None) == 0
    empty = gpu.torch.zeros((0, 2), dtype=gpu.torch.float32, device="cuda")
    assert ctx.get_watermark_batch(None, [empty, x], sample_rate=R48)[0] == []
