"""Whole streams from and to signed 16-bit PCM (awm_add_watermark_s16_d and its twins), without a GPU: the entry
points are exported, declared next to their float twins and have argument types, every entry point answers "null context" before anything
else and leaves its outputs alone, no profiling scope was added, and the binding has the methods while the float methods keep their
signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import audiowmark_amd as awm

SYMBOLS = ("awm_add_mix_s16_d", "awm_add_limit_s16_d", "awm_add_watermark_s16_d", "awm_add_get_watermark_s16_d",
           "awm_debug_add_s16_fused_in_use")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "awm_hip.h")


def declaration(header, name):
    m = re.search(r"\b%s \(([^;]*)\);" % re.escape(name), header)
    assert m, name
    return " ".join(m.group(1).split())


def test_symbols_are_exported_and_declared():
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert hasattr(awm.lib, name), name
        assert getattr(awm.lib, name).argtypes is not None, name
        declaration(header, name)
    assert declaration(header, "awm_add_mix_s16_d").startswith(
        "awm_ctx *ctx, const int16_t *pcm_in_d, float *out_d, size_t n_frames, int n_channels, const int8_t *frame_mod, double water_delta, "
        "size_t first_frame, const int16_t *halo_before_d, const int16_t *halo_after_d, float *block_max_d")
    assert declaration(header, "awm_add_limit_s16_d").startswith(
        "awm_ctx *ctx, const float *mix_d, int16_t *out_d, size_t n_frames, int n_channels, size_t first_sample, const float *block_max_d")
    assert declaration(header, "awm_add_watermark_s16_d") == (
        "awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const int16_t *pcm_in_d, int16_t *out_d, size_t n_frames, "
        "int n_channels, int sample_rate")
    assert declaration(header, "awm_add_get_watermark_s16_d") == (
        "awm_ctx *ctx, const uint8_t key[16], const char *payload_hex, const int16_t *pcm_in_d, int16_t *out_d, size_t n_frames, "
        "int n_channels, int sample_rate, size_t max_out, awm_pattern *out")
    assert declaration(header, "awm_debug_add_s16_fused_in_use") == "void"
    # next to their float twins
    assert header.index("int awm_add_limit_d (") < header.index("int awm_add_mix_s16_d (") < header.index("int awm_add_d (")
    assert header.index("int awm_add_get_watermark_d (") < header.index("int awm_add_watermark_s16_d (") < header.index("int awm_get_watermark_keys_d (")
    # the twins take their float twins' argument lists
    assert len(awm.lib.awm_add_mix_s16_d.argtypes) == len(awm.lib.awm_add_mix_d.argtypes)
    assert len(awm.lib.awm_add_limit_s16_d.argtypes) == len(awm.lib.awm_add_limit_d.argtypes) + 1
    assert len(awm.lib.awm_add_watermark_s16_d.argtypes) == len(awm.lib.awm_add_watermark_d.argtypes)
    assert len(awm.lib.awm_add_get_watermark_s16_d.argtypes) == len(awm.lib.awm_add_get_watermark_d.argtypes)
    # what is left out is said
    assert "Not offered from 16-bit input: many payloads" in header
    # ... and the `get` side no longer lists what now exists
    assert "the `add` side for whole streams;" not in header


def test_no_profiling_scope_was_added():
    awm.lib.awm_prof_name.restype = C.c_char_p
    names = [awm.lib.awm_prof_name(i).decode() for i in range(awm.lib.awm_prof_count())]
    assert len(names) == 33
    for name in ("add_mix_kernel", "limit_encode_s16_kernel", "resample_s16_kernel", "pcm_decode_kernel", "pcm_encode_kernel", "limiter_kernel"):
        assert names.count(name) == 1, (name, names)


def test_entry_points_need_a_context():
    lib = awm.lib
    pats = np.full(4096, 0x5a, np.uint8)
    out16 = np.full(64, 0x5a5a, np.uint16)
    outf = np.full(64, -7.0, np.float32)
    bm = np.full(4, -7.0, np.float32)
    fm = np.zeros(2 * 2226 * 81, np.int8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    key = bytes(16)
    pay = b"0123456789abcdef0011223344556677"
    for ptr in (None, C.c_void_p(3), C.c_void_p(4096)):
        calls = (lambda: lib.awm_add_mix_s16_d(None, ptr, vp(outf), 16, 2, vp(fm), 0.01, 0, None, None, vp(bm), 0, 4),
                 lambda: lib.awm_add_limit_s16_d(None, vp(outf), vp(out16), 16, 2, 0, vp(bm), 0, 4),
                 lambda: lib.awm_add_watermark_s16_d(None, key, pay, ptr, vp(out16), 16, 2, 44100),
                 lambda: lib.awm_add_watermark_s16_d(None, key, pay, ptr, vp(out16), 16, 2, 48000),
                 lambda: lib.awm_add_watermark_s16_d(None, key, pay, ptr, vp(out16), 16, 2, -1),
                 lambda: lib.awm_add_get_watermark_s16_d(None, key, pay, ptr, vp(out16), 16, 2, 44100, 8, vp(pats)),
                 lambda: lib.awm_add_get_watermark_s16_d(None, key, b"xyz", ptr, vp(out16), 16, 2, 48000, 8, None))
        for call in calls:
            assert call() < 0
            assert b"null context" in lib.awm_last_error()
    assert (pats == 0x5a).all() and (out16 == 0x5a5a).all() and (outf == -7).all() and (bm == -7).all()
    assert lib.awm_debug_add_s16_fused_in_use() in (0, 1)
    assert lib.awm_debug_lane_add_mix_bytes(None) == 0


def test_the_binding_has_the_methods():
    s16 = {"add_watermark_s16": ["self", "key", "payload_hex", "pcm16", "out", "sample_rate"],
           "add_get_watermark_s16": ["self", "key", "payload_hex", "pcm16", "out", "sample_rate"],
           "add_mix_s16": ["self", "pcm16", "out", "frame_mod", "water_delta", "first_frame", "halo_before", "halo_after", "block_max", "first_block"],
           "add_limit_s16": ["self", "mix", "out", "first_sample", "block_max", "first_block"]}
    for name, params in s16.items():
        assert list(inspect.signature(getattr(awm.Context, name)).parameters) == params, name
    sig = inspect.signature(awm.Context.add_watermark_s16).parameters
    assert sig["out"].default is None and sig["sample_rate"].default == 44100
    assert inspect.signature(awm.Context.add_get_watermark_s16).parameters["sample_rate"].default == 44100
    # the float methods keep their signatures
    floats = {"add_watermark": ["self", "key", "payload_hex", "pcm", "out", "sample_rate"],
              "add_get_watermark": ["self", "key", "payload_hex", "pcm", "out", "sample_rate"],
              "add_mix": ["self", "pcm", "out", "frame_mod", "water_delta", "first_frame", "halo_before", "halo_after", "block_max", "first_block"],
              "add_limit": ["self", "out", "first_sample", "block_max", "first_block"],
              "get_watermark_s16": ["self", "key", "pcm16", "sample_rate"]}
    for name, params in floats.items():
        assert list(inspect.signature(getattr(awm.Context, name)).parameters) == params, name
