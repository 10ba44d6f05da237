"""Clip batches with a sample rate per clip (awm_get_watermark_batch_rates_d and its twins), without a GPU: the
entry points are exported and declared, the profiling scope of K10x is there under its name beside K10c's, the device entry points refuse
to run without a context (no CPU fallback), the pure-host plan sends every clip the way the batch will send it, and the binding's keyword
keeps its default and takes a sequence."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import audiowmark_amd as awm

SYMBOLS = ("awm_get_watermark_batch_rates_d", "awm_get_watermark_batch_keys_rates_d", "awm_debug_clip_stage_rates_d",
           "awm_get_batch_rates_plan")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "awm_hip.h")
ERR_ARG = -3            # AWM_ERR_ARG (include/awm_hip.h)
GROUP, LANE_FIXED, LANE_VAR, EMPTY = 0, 1, 2, 3


def test_symbols_are_exported_and_declared():
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert hasattr(awm.lib, name), name
        assert name + " (" in header, name
    assert "get_batch_rates_plan" in awm.__all__


def test_profiling_names():
    awm.lib.awm_prof_name.restype = C.c_char_p
    names = [awm.lib.awm_prof_name(i).decode() for i in range(awm.lib.awm_prof_count())]
    assert names.count("clip_stage_mixed_kernel") == 1
    assert names.count("clip_resample_pad_kernel") == 1
    assert all(names)


def test_entry_points_need_a_context():
    lib = awm.lib
    ptrs = (C.c_void_p * 2)(None, None)
    frames = (C.c_size_t * 2)(1024, 1024)
    n_out = (C.c_int * 2)(-7, -7)
    rng = np.full((2, 2), -7, np.int64)
    for rates in ((C.c_int * 2)(48000, 32000), (C.c_int * 2)(48000, 48000), (C.c_int * 2)(44100, 44100)):       # mixed, and the two that forward
        calls = (lambda: lib.awm_get_watermark_batch_rates_d(None, bytes(16), 2, ptrs, frames, 2, rates, 0, 0, None, n_out),
                 lambda: lib.awm_get_watermark_batch_keys_rates_d(None, bytes(32), 2, ptrs, frames, 2, rates, 0, 0, None, n_out),
                 lambda: lib.awm_debug_clip_stage_rates_d(None, 2, ptrs, frames, 2, rates, None, rng.ctypes.data_as(C.c_void_p)))
        for call in calls:
            assert call() < 0
            assert b"null context" in lib.awm_last_error()
    assert list(n_out) == [-7, -7] and (rng == -7).all()


def border():
    """first 44.1 kHz length that is long: (block frames + 2) 1024"""
    return (awm.lib.awm_debug_clip_slice_values(1) // 3072 - 5 + 2) * 1024


def frames_48k_for(n44):
    """the smallest 48 kHz length whose 44.1 kHz length reaches n44 (the ratio is below 1: it has exactly n44)"""
    n = max(1, n44 * 48000 // 44100 - 2)
    while awm.get_batch_rates_plan([n], [48000])[1][0] < n44:
        n += 1
    return n


def test_plan_paths():
    b = border()
    assert b > 44100 * 50
    paths, n44 = awm.get_batch_rates_plan([1, 5000, b - 1, b], [44100] * 4)
    assert list(n44) == [1, 5000, b - 1, b]
    assert list(paths) == [GROUP, GROUP, GROUP, LANE_FIXED]
    lengths = [frames_48k_for(b - 1), frames_48k_for(b)]
    paths, n44 = awm.get_batch_rates_plan(lengths, [48000, 48000])
    assert list(n44) == [b - 1, b]
    assert list(paths) == [GROUP, LANE_FIXED]
    paths, n44 = awm.get_batch_rates_plan([5000, 0, 0, 70 * 33333], [33333, 48000, 44100, 33333])
    assert list(paths) == [LANE_VAR, EMPTY, EMPTY, LANE_VAR]
    assert n44[0] > 0 and n44[1] == 0 and n44[2] == 0
    # the six rates of a detection queue, one short clip each: all in the groups, lengths within a frame of the ratio
    rates = [44100, 48000, 32000, 96000, 22050, 88200]
    paths, n44 = awm.get_batch_rates_plan([r * 3 for r in rates], rates)
    assert list(paths) == [GROUP] * 6
    assert all(abs(int(n) - 3 * 44100) <= 1 for n in n44)
    assert awm.get_batch_rates_plan([], []) [0].size == 0


@pytest.mark.parametrize("bad", [0, -1, 1000000])
@pytest.mark.parametrize("at", [0, 2])
def test_plan_refuses(bad, at):
    lib = awm.lib
    rates = [48000, 44100, 32000]
    rates[at] = bad
    c_rates = (C.c_int * 3)(*rates)
    frames = (C.c_size_t * 3)(5000, 6000, 7000)
    paths = (C.c_int * 3)(-9, -9, -9)
    n44 = (C.c_size_t * 3)()
    assert lib.awm_get_batch_rates_plan(3, frames, c_rates, paths, n44) == ERR_ARG
    assert b"clip %d:" % at in lib.awm_last_error()
    assert paths[at] == -1
    assert [p for i, p in enumerate(paths) if i != at] == [GROUP, GROUP]
    with pytest.raises(awm.AwmError):
        awm.get_batch_rates_plan([5000, 6000, 7000], rates)
    assert lib.awm_get_batch_rates_plan(3, frames, None, paths, n44) == ERR_ARG


def test_the_keyword_defaults_to_44100_and_takes_a_sequence():
    for fn in (awm.Context.get_watermark_batch, awm.Context.get_watermark_batch_keys):
        assert inspect.signature(fn).parameters["sample_rate"].default == 44100
    assert "sample_rate" in inspect.signature(awm.Context.clip_stage).parameters
    from audiowmark_amd.binding import _rates_array
    assert _rates_array(48000, 3) is None and _rates_array(np.int64(48000), 3) is None
    for seq in ([48000, 44100, 32000], (48000, 44100, 32000), np.array([48000, 44100, 32000])):
        arr = _rates_array(seq, 3)
        assert isinstance(arr, C.Array) and list(arr) == [48000, 44100, 32000]
    with pytest.raises(ValueError):
        _rates_array([48000], 3)
