"""Whole streams straight from signed 16-bit PCM (awm_get_watermark_s16_d and its twins), without a GPU: the
entry points are exported and declared, the profiling scopes of the 16-bit kernels are there once each behind all the scopes that
existed, every entry point answers "null context" before anything else and leaves its outputs alone, and the binding has the methods
while the float methods keep their signatures."""
import ctypes as C
import inspect
import os

import numpy as np

import audiowmark_amd as awm

PIPELINE = ("awm_get_watermark_s16_d", "awm_get_watermark_keys_s16_d", "awm_get_watermark_rate_s16_d")
KERNEL_LEVEL = ("awm_sync_fft_s16_d", "awm_sync_search_s16_d", "awm_block_soft_bits_s16_d", "awm_debug_sync_db_sliding_rows_s16_d")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "awm_hip.h")
NEW_SCOPES = ("sync_db_s16_kernel(approx)", "sync_db_s16_kernel(refine)", "sync_db_s16_kernel(block)", "resample_s16_kernel")
# the last scope of the parent: everything new comes behind it
LAST_OLD_SCOPE = "limit_encode_s16_kernel"
OLD_SCOPES = ("sync_db_kernel(approx)", "sync_db_kernel(refine)", "sync_db_kernel(block)", "resample_kernel", "pcm_decode_kernel",
              "clip_pad_s16_kernel", "clip_resample_pad_s16_kernel", "clip_stage_mixed_s16_kernel", "segment_gather_s16_kernel", LAST_OLD_SCOPE)


def test_symbols_are_exported_and_declared():
    header = open(HEADER).read()
    for name in PIPELINE + KERNEL_LEVEL:
        assert hasattr(awm.lib, name), name
        assert name + " (" in header, name
        assert getattr(awm.lib, name).argtypes is not None, name
    for name in PIPELINE + KERNEL_LEVEL:
        decl = header[header.index(name + " ("):]
        assert "const int16_t *pcm_d" in decl[:decl.index(";")], name
    # the header says what only the default forms offer and what is left out
    assert "only the default" in header and "awm_debug_set_refine_form" in header
    assert "Not offered: the file level and the command line" in header


def test_profiling_names():
    awm.lib.awm_prof_name.restype = C.c_char_p
    names = [awm.lib.awm_prof_name(i).decode() for i in range(awm.lib.awm_prof_count())]
    assert all(names)
    for name in NEW_SCOPES + OLD_SCOPES:
        assert names.count(name) == 1, name
    # appended: the scopes that were there keep their numbers
    assert names.index(LAST_OLD_SCOPE) == 28
    assert sorted(names.index(n) for n in NEW_SCOPES) == list(range(29, 29 + len(NEW_SCOPES)))
    assert len(names) == 29 + len(NEW_SCOPES)


def test_entry_points_need_a_context():
    lib = awm.lib
    pats = np.full(4096, 0x5a, np.uint8)
    which = np.full(8, -7, np.int32)
    idx = np.full(8, 77, np.uint64)
    q = np.full(8, -7.0)
    bt = np.full(8, -7, np.int32)
    soft = np.full(858 * 2, -7.0, np.float32)
    ok = np.full(2, -7, np.int32)
    blocks = np.zeros(2, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    key = bytes(16)
    for ptr in (None, C.c_void_p(3), C.c_void_p(4096)):
        calls = (lambda: lib.awm_get_watermark_s16_d(None, key, ptr, 4096, 2, 8, vp(pats)),
                 lambda: lib.awm_get_watermark_keys_s16_d(None, bytes(32), 2, ptr, 4096, 2, 8, vp(pats), vp(which)),
                 lambda: lib.awm_get_watermark_rate_s16_d(None, key, ptr, 4096, 2, 48000, 8, vp(pats)),
                 lambda: lib.awm_get_watermark_rate_s16_d(None, key, ptr, 4096, 2, 44100, 8, vp(pats)),
                 lambda: lib.awm_get_watermark_rate_s16_d(None, key, ptr, 4096, 2, -1, 8, vp(pats)),
                 lambda: lib.awm_sync_fft_s16_d(None, ptr, 4096, 2, 0, 2, None, 0, 8192, None, None),
                 lambda: lib.awm_sync_search_s16_d(None, key, ptr, 4096, 2, 1, 8, vp(idx), vp(q), vp(bt)),
                 lambda: lib.awm_block_soft_bits_s16_d(None, key, ptr, 4096, 2, vp(blocks), 2, vp(soft), vp(ok)),
                 lambda: lib.awm_debug_sync_db_sliding_rows_s16_d(None, ptr, 4096, 2, None, None, 1, 1, 1, None, None, 0, 8192, None, None, 1, 0, 72,
                                                                  None, None, 0, None, 72))
        for call in calls:
            assert call() < 0
            assert b"null context" in lib.awm_last_error()
    assert (pats == 0x5a).all() and (which == -7).all() and (idx == 77).all() and (q == -7).all() and (bt == -7).all()
    assert (soft == -7).all() and (ok == -7).all()
    assert lib.awm_debug_lane_pcm_bytes(None) == 0


def test_the_binding_has_the_methods():
    s16 = {"get_watermark_s16": ["self", "key", "pcm16", "sample_rate"], "get_watermark_keys_s16": ["self", "keys", "pcm16"],
           "sync_fft_s16": ["self", "pcm16", "index", "frame_count", "want_frames", "first", "last", "out"],
           "sync_search_s16": ["self", "key", "pcm16", "clip_mode", "max_out"], "block_soft_bits_s16": ["self", "key", "pcm16", "indices"]}
    for name, params in s16.items():
        assert list(inspect.signature(getattr(awm.Context, name)).parameters) == params, name
    assert inspect.signature(awm.Context.get_watermark_s16).parameters["sample_rate"].default == 44100
    # the rows call: the float method's parameters with the stream renamed
    rows = list(inspect.signature(awm.Context.sync_db_sliding_rows).parameters)
    assert list(inspect.signature(awm.Context.sync_db_sliding_rows_s16).parameters) == ["self", "pcm16"] + rows[2:]
    # the float methods keep their signatures
    floats = {"get_watermark": ["self", "key", "pcm", "sample_rate"], "get_watermark_keys": ["self", "keys", "pcm"],
              "sync_fft": ["self", "pcm", "index", "frame_count", "want_frames", "first", "last", "out"],
              "sync_search": ["self", "key", "pcm", "clip_mode", "max_out"], "block_soft_bits": ["self", "key", "pcm", "indices"]}
    for name, params in floats.items():
        assert list(inspect.signature(getattr(awm.Context, name)).parameters) == params, name
    assert rows[:4] == ["self", "pcm", "n_frames", "bases"]
