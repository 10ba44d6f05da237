"""Segments with a key each (awm_add_watermark_segments_keys_d / _rate_d), without a GPU: the symbols are exported and
declared, K16t has a profiling id named as rocprofv3 shows the kernel, and the entry points refuse to run without a context -- there is no
CPU fallback -- before they look at anything else, as every entry point that takes a context does (check_ctx: "null context")."""
import ctypes as C
import os

import pytest

import audiowmark_amd as awm
from audiowmark_amd import binding

SYMBOLS = ["awm_add_watermark_segments_keys_d", "awm_add_watermark_segments_keys_rate_d", "awm_debug_key_templates_d",
           "awm_debug_key_payload_tables_d"]
ERR_NO_DEVICE, ERR_ARG = -2, -3


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_are_exported_and_declared(name):
    assert getattr(awm.lib, name) is not None
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "awm_hip.h")) as f:
        assert name + " (" in f.read()


def test_the_binding_offers_the_calls():
    for name in ("add_watermark_segments_keys", "key_templates", "key_payload_tables"):
        assert callable(getattr(awm.Context, name))


def test_the_template_kernel_has_a_profiling_id():
    awm.lib.awm_prof_name.restype = C.c_char_p
    names = [awm.lib.awm_prof_name(i).decode() for i in range(awm.lib.awm_prof_count())]
    assert names.count("key_template_kernel") == 1
    assert "frame_mod_table_kernel" in names and "payload_table_kernel" in names          # (K16 and K16p keep theirs)


def test_the_header_names_the_new_functions_where_it_said_not_offered():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "awm_hip.h")) as f:
        text = f.read()
    assert ", a key per segment. */" not in text
    assert text.count("A key per segment:") == 2


def calls():
    n = 2
    keys = bytes(16) + awm.test_key(7)
    hexes = (C.c_char_p * n)(b"0123456789abcdef0011223344556677", b"f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0")
    zf = (C.c_size_t * n)(0, 1024)
    ptrs = (C.c_void_p * n)(None, None)
    frames = (C.c_size_t * n)(0, 0)
    lib = awm.lib
    return {
        "awm_add_watermark_segments_keys_d": lambda ctx: lib.awm_add_watermark_segments_keys_d(ctx, keys, n, hexes, zf, ptrs, ptrs, frames, 2),
        "awm_add_watermark_segments_keys_d (one key)": lambda ctx: lib.awm_add_watermark_segments_keys_d(ctx, bytes(32), n, hexes, zf, ptrs, ptrs, frames, 2),
        "awm_add_watermark_segments_keys_d (no keys)": lambda ctx: lib.awm_add_watermark_segments_keys_d(ctx, None, n, hexes, zf, ptrs, ptrs, frames, 2),
        "awm_add_watermark_segments_keys_d (no segments)": lambda ctx: lib.awm_add_watermark_segments_keys_d(ctx, None, 0, None, None, None, None, None, 2),
        "awm_add_watermark_segments_keys_rate_d": lambda ctx: lib.awm_add_watermark_segments_keys_rate_d(ctx, keys, n, hexes, zf, ptrs, ptrs, frames, 2, 48000),
        "awm_add_watermark_segments_keys_rate_d (44100)": lambda ctx: lib.awm_add_watermark_segments_keys_rate_d(ctx, keys, n, hexes, zf, ptrs, ptrs, frames, 2, 44100),
        "awm_add_watermark_segments_keys_rate_d (44101)": lambda ctx: lib.awm_add_watermark_segments_keys_rate_d(ctx, keys, n, hexes, zf, ptrs, ptrs, frames, 2, 44101),
        "awm_debug_key_templates_d": lambda ctx: lib.awm_debug_key_templates_d(ctx, keys, n, None),
        "awm_debug_key_payload_tables_d": lambda ctx: lib.awm_debug_key_payload_tables_d(ctx, keys, hexes, n, None),
    }


@pytest.mark.parametrize("what", sorted(calls()))
def test_entry_points_need_a_context(what):
    """the context is looked at first: AWM_ERR_ARG "null context" whatever the other arguments are, good or bad"""
    rc = calls()[what](None)
    assert rc == ERR_ARG, what
    assert b"null context" in awm.lib.awm_last_error(), what
    with pytest.raises(awm.AwmError):
        binding._check(rc, what)


def test_no_device_no_context():
    """... and without a device there is no context to give them: awm_ctx_create says AWM_ERR_NO_DEVICE (tests/test_host_abi.py)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    assert awm.lib.awm_ctx_create(0, C.byref(h)) == ERR_NO_DEVICE
    assert not h.value
