"""Stage 0 of a group of 44.1 kHz clips -- the copy form -- against slices built from the definition.

Every other bit test of stage 0 ends in the copy stage: a stage at a rate is held to "resample, then the 44.1 kHz stage", the 16-bit stage to
the float stage.  Here the 44.1 kHz stage itself is held to what kernels.hh says it writes, for float and for 16-bit clips:

  a slice has V = awm_debug_clip_slice_values (ch) values, n = V / 3; a clip of L = frames * ch values sits at pad_start = 2 n - L;
  the written window is [lo, hi) with lo = max (0, (pad_start - 2048 ch) / 4 * 4), hi = min (V, (pad_start + L + 2048 ch + 3) / 4 * 4):
  zeros and the clip inside it, and outside it whatever the buffer held (canaries; NaN bits under awm_debug_set_clip_poison);
  the range of slice i is (i V + pad_start + first non-zero, i V + pad_start + last non-zero + 1), or (-1, 0) for a silent clip;
  a 16-bit value v is float (v) * 2^-15, which is exact.

Values are compared as int32, there is no tolerance.  The lengths are those of test_gpu_get_rate.py: 1, 2 and the neighbours of 1024 and
2352 values reach the rounding to quads at both edges of the window with every remainder, the long clips several workgroups per slice and
the range atomics.  expected_slices is itself checked (without a GPU) against a restatement of the kernel's loop over quads."""
import numpy as np
import pytest
import torch

from _placement import CANARY
from test_gpu_get_rate import GROUPS, MATERIALS, cached, gpu, material      # noqa: F401 (gpu: the fixture)

MARGIN_FRAMES = 2048
POISON = -1             # 0xffffffff, what awm_debug_set_clip_poison fills the slices with


def as_float(values):
    """the float32 values stage 0 stores for a clip's values (float32 as they are, int16 times 2^-15)"""
    return values if values.dtype == torch.float32 else values.to(torch.float32) * (1.0 / 32768.0)


def expected_slices(clips, ch, slice_values, outside):
    """([n_clips, slice_values] int32, [n_clips, 2] int64) from the definition above; clips: tensors of L values each, float32 or int16"""
    n = slice_values // 3
    exp = torch.full((len(clips), slice_values), outside, dtype=torch.int32, device=clips[0].device)
    ranges = np.zeros((len(clips), 2), np.int64)
    for i, c in enumerate(clips):
        x = as_float(c.reshape(-1))
        length = x.numel()
        pad_start = 2 * n - length
        lo = max(0, (pad_start - MARGIN_FRAMES * ch) // 4 * 4)
        hi = min(slice_values, (pad_start + length + MARGIN_FRAMES * ch + 3) // 4 * 4)
        exp[i, lo:hi] = 0
        exp[i, pad_start:pad_start + length] = x.view(torch.int32)
        nonzero = torch.nonzero(x != 0).reshape(-1)
        if nonzero.numel():
            ranges[i] = (i * slice_values + pad_start + int(nonzero[0]), i * slice_values + pad_start + int(nonzero[-1]) + 1)
        else:
            ranges[i] = (-1, 0)
    return exp, ranges


def kernel_restated(clips, ch, slice_values, outside):
    """the copy kernel's index arithmetic in numpy: quads q_lo .. q_hi of a slice, value j of quad q from source index 4 q - pad_start + j"""
    out = np.full((len(clips), slice_values), outside, np.int32)
    ranges = np.zeros((len(clips), 2), np.int64)
    margin = MARGIN_FRAMES * ch
    for i, c in enumerate(clips):
        data = as_float(c.reshape(-1)).numpy()
        n_values = data.size
        pad_start = slice_values // 3 + (slice_values // 3 - n_values)
        q_lo = max(0, int((pad_start - margin) / 4))                    # (C++ division: towards zero)
        q_hi = min(slice_values // 4, (pad_start + n_values + margin + 3) // 4)
        q = np.arange(q_lo, q_hi, dtype=np.int64)[:, None]
        k = 4 * q - pad_start + np.arange(4)                            # source index of value j of quad q
        inside = (k >= 0) & (k < n_values)
        v = np.where(inside, data[np.clip(k, 0, n_values - 1)], np.float32(0)).astype(np.float32)
        out[i, 4 * q_lo:4 * q_hi] = v.reshape(-1).view(np.int32)
        at = (i * slice_values + 4 * q + np.arange(4))[v != 0]
        ranges[i] = (at.min(), at.max() + 1) if at.size else (-1, 0)
    return out, ranges


@pytest.mark.parametrize("ch", [1, 2, 3])
def test_expected_slices_are_the_kernels_arithmetic(ch):
    """(no GPU) small slices: a margin that is clipped at both ends of the slice (n < 2048 ch), one that is not, every remainder of
    pad_start and of the clip's end modulo 4, silent clips, first / last value only, float and 16-bit"""
    rng = np.random.default_rng(40 + ch)
    for n in (8 * ch, 1024 * ch, 2600 * ch):
        n = (n + 3) // 4 * 4
        lengths = [f for f in (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025) if f * ch <= n] + [n // ch]
        for dtype in (torch.float32, torch.int16):
            clips = []
            for k, frames in enumerate(lengths):
                x = rng.uniform(-1, 1, frames * ch).astype(np.float32)
                if k % 4 == 1:
                    x[:] = 0
                elif k % 4 == 2:
                    x[1:] = 0
                elif k % 4 == 3:
                    x[:-1] = 0
                clips.append(torch.from_numpy(x) if dtype == torch.float32 else torch.from_numpy(np.round(x * 32767).astype(np.int16)))
            exp, exp_rng = expected_slices(clips, ch, 3 * n, CANARY)
            got, got_rng = kernel_restated(clips, ch, 3 * n, CANARY)
            assert np.array_equal(exp.numpy(), got)
            assert np.array_equal(exp_rng, got_rng), (exp_rng, got_rng)


def to_s16(x):
    return torch.round(x * 32767).to(torch.int16)


def shifted(x, values):
    """a copy of the clip that begins `values` values of its type behind an allocation's (at least 16-byte aligned) start"""
    flat = torch.empty(x.numel() + values, dtype=x.dtype, device=x.device)
    flat[values:] = x.reshape(-1)
    return flat[values:].view(x.shape)


def stage_copy_check(gpu, clips, ch, outside):
    """one stage call on float32 or int16 clips into a buffer full of canaries against expected_slices, on the device"""
    t = gpu.torch
    values = gpu.lib.awm_debug_clip_slice_values(ch)
    assert values > 0 and values % 12 == 0
    buf = cached(("copy canary", len(clips), values), lambda: t.empty((len(clips), values), dtype=t.float32, device="cuda"))
    buf.view(t.int32).fill_(CANARY)
    if clips[0].dtype == t.int16:
        got, got_rng = gpu.ctx.clip_stage_s16(clips, 44100, out=buf)
    else:
        got, got_rng = gpu.ctx.clip_stage(clips, 44100, out=buf)
    exp, exp_rng = expected_slices(clips, ch, values, outside)
    assert bool((got.view(t.int32) == exp).all()), "a value of the padded slices differs from the definition"
    assert np.array_equal(got_rng, exp_rng), (got_rng, exp_rng)
    return got_rng


def group_clips(gpu, group, gi, kind, ch, s16):
    """the clips of one stage call; the second one and the last, longest one begin 4 bytes off a 16-byte boundary (float) or 2 bytes off a
    4-byte boundary (int16)"""
    clips = [material(gpu, kind, 900 + 10 * gi + i, n, ch) for i, n in enumerate(group)]
    if s16:
        clips = [to_s16(c) for c in clips]
    for i in (1, len(clips) - 1):
        clips[i] = shifted(clips[i], 1)
        assert clips[i].data_ptr() % (4 if s16 else 16) == (2 if s16 else 4)
    return clips


@pytest.mark.gpu
@pytest.mark.parametrize("s16", [False, True], ids=["float", "s16"])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_copy_stage_is_the_definition(gpu, ch, s16):
    for gi, group in enumerate(GROUPS):
        for kind in MATERIALS:
            rng = stage_copy_check(gpu, group_clips(gpu, group, gi, kind, ch, s16), ch, CANARY)
            if kind == "zero":
                assert all(tuple(r) == (-1, 0) for r in rng)
            elif kind == "noise":
                assert all(r[0] >= 0 and r[1] > r[0] for r in rng)


@pytest.mark.gpu
@pytest.mark.parametrize("s16", [False, True], ids=["float", "s16"])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_copy_stage_under_poison(gpu, ch, s16):
    """the launcher fills the slices with NaN bits first: the window is as before, everything outside it is no longer the canary"""
    gpu.lib.awm_debug_set_clip_poison(1)
    try:
        for gi, group in enumerate(GROUPS):
            for kind in ("noise", "fifth", "last", "zero"):
                stage_copy_check(gpu, group_clips(gpu, group, gi, kind, ch, s16), ch, POISON)
    finally:
        gpu.lib.awm_debug_set_clip_poison(0)
