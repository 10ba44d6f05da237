"""`get` on resident material at sample rates other than 44.1 kHz, without a GPU: the entry points and the debug stage are exported, the
profiling id of K10c is there under the kernel's name, the entry points refuse to run without a context at 48 kHz (there is no CPU
fallback), and the binding's new keyword keeps every existing call at 44.1 kHz."""
import ctypes as C
import inspect

import audiowmark_amd as awm

SYMBOLS = ("awm_get_watermark_rate_d", "awm_get_watermark_batch_rate_d", "awm_get_watermark_batch_keys_rate_d",
           "awm_debug_clip_slice_values", "awm_debug_clip_stage_d")


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert hasattr(awm.lib, name), name


def test_profiling_id_of_the_new_kernel():
    awm.lib.awm_prof_name.restype = C.c_char_p
    names = [awm.lib.awm_prof_name(i).decode() for i in range(awm.lib.awm_prof_count())]
    assert names.count("clip_resample_pad_kernel") == 1
    assert "resample_kernel" in names and all(names)


def test_entry_points_need_a_context_at_48_khz():
    lib = awm.lib
    ptrs = (C.c_void_p * 1)(None)
    frames = (C.c_size_t * 1)(1024)
    n_out = (C.c_int * 1)(-7)
    calls = (lambda: lib.awm_get_watermark_rate_d(None, bytes(16), None, 1024, 2, 48000, 0, None),
             lambda: lib.awm_get_watermark_batch_rate_d(None, bytes(16), 1, ptrs, frames, 2, 48000, 0, 0, None, n_out),
             lambda: lib.awm_get_watermark_batch_keys_rate_d(None, bytes(16), 1, ptrs, frames, 2, 48000, 0, 0, None, n_out))
    for call in calls:
        assert call() < 0
        assert b"null context" in lib.awm_last_error()
    assert n_out[0] == -7


def test_the_keyword_defaults_to_44100():
    for fn in (awm.Context.get_watermark, awm.Context.get_watermark_batch, awm.Context.get_watermark_batch_keys):
        assert inspect.signature(fn).parameters["sample_rate"].default == 44100
    assert "sample_rate" in inspect.signature(awm.Context.clip_stage).parameters
