"""Clip batches straight from signed 16-bit PCM (awm_get_watermark_batch_rates_s16_d and its twins), without a GPU:
the entry points are exported and declared, the profiling scopes of the 16-bit stage 0 are there under names of their own beside the
float ones, the device entry points refuse to run without a context (no CPU fallback; the context check comes first, so the refusals of
pointers and rates are in tests/test_gpu_get_s16.py), and the binding has the three methods with the keyword's default."""
import ctypes as C
import inspect
import os

import numpy as np

import audiowmark_amd as awm

SYMBOLS = ("awm_get_watermark_batch_rates_s16_d", "awm_get_watermark_batch_keys_rates_s16_d", "awm_debug_clip_stage_rates_s16_d")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "awm_hip.h")
S16_SCOPES = ("clip_pad_s16_kernel", "clip_resample_pad_s16_kernel", "clip_stage_mixed_s16_kernel")
FLOAT_SCOPES = ("clip_resample_pad_kernel", "clip_stage_mixed_kernel", "resample_kernel", "resample_var_kernel")


def test_symbols_are_exported_and_declared():
    header = open(HEADER).read()
    for name in SYMBOLS + ("awm_debug_lane_pcm_bytes",):
        assert hasattr(awm.lib, name), name
        assert name + " (" in header, name
    for name in SYMBOLS:
        assert getattr(awm.lib, name).argtypes is not None, name
    # the header says what the form leaves out, and that the plan holds for it
    assert "const int16_t *const *pcm_d" in header
    assert "The 16-bit batches below take the same paths" in header


def test_profiling_names():
    awm.lib.awm_prof_name.restype = C.c_char_p
    names = [awm.lib.awm_prof_name(i).decode() for i in range(awm.lib.awm_prof_count())]
    for name in S16_SCOPES + FLOAT_SCOPES:
        assert names.count(name) == 1, name
    assert all(names)
    # appended: the scopes that were there keep their numbers
    assert min(names.index(n) for n in S16_SCOPES) > names.index("clip_stage_mixed_kernel")


def test_entry_points_need_a_context():
    lib = awm.lib
    ptrs = (C.c_void_p * 2)(None, None)
    odd = (C.c_void_p * 2)(3, 5)
    frames = (C.c_size_t * 2)(1024, 1024)
    n_out = (C.c_int * 2)(-7, -7)
    rng = np.full((2, 2), -7, np.int64)
    for rates in ((C.c_int * 2)(48000, 32000), (C.c_int * 2)(48000, 48000), (C.c_int * 2)(44100, 44100), (C.c_int * 2)(-1, 48000), None):
        for p in (ptrs, odd):
            calls = (lambda: lib.awm_get_watermark_batch_rates_s16_d(None, bytes(16), 2, p, frames, 2, rates, 0, 0, None, n_out),
                     lambda: lib.awm_get_watermark_batch_keys_rates_s16_d(None, bytes(32), 2, p, frames, 2, rates, 0, 0, None, n_out),
                     lambda: lib.awm_debug_clip_stage_rates_s16_d(None, 2, p, frames, 2, rates, None, rng.ctypes.data_as(C.c_void_p)))
            for call in calls:
                assert call() < 0
                assert b"null context" in lib.awm_last_error()
    assert list(n_out) == [-7, -7] and (rng == -7).all()
    assert lib.awm_debug_lane_pcm_bytes(None) == 0


def test_the_binding_has_the_methods():
    for fn in (awm.Context.get_watermark_batch_s16, awm.Context.get_watermark_batch_keys_s16, awm.Context.clip_stage_s16):
        assert inspect.signature(fn).parameters["sample_rate"].default == 44100
    # the float methods keep their signatures
    for fn in (awm.Context.get_watermark_batch, awm.Context.get_watermark_batch_keys):
        assert list(inspect.signature(fn).parameters)[-3:] == ["n_threads", "max_out_per_clip", "sample_rate"]
    assert inspect.signature(awm.Context.clip_stage).parameters["sample_rate"].default is inspect.Parameter.empty
