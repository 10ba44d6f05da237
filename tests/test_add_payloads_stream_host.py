"""Many payloads through a span, the tile stream and files, without a GPU: the symbols are exported, the entry points refuse to run
without a context (there is no CPU fallback), and the binding's list and path checks raise before the library is called."""
import ctypes as C
import os

import pytest
import torch

import audiowmark_amd as awm
from audiowmark_amd import binding

PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"
SYMBOLS = ["awm_add_mix_payloads_d", "awm_add_stream_create_payloads_at", "awm_add_stream_payloads", "awm_add_stream_push_payloads",
           "awm_add_watermark_payloads_file", "awm_add_stream_watermark_payloads_file", "awm_debug_set_payloads_file_tile"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_are_exported_and_declared(name):
    assert getattr(awm.lib, name) is not None
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "awm_hip.h")) as f:
        assert name + " (" in f.read()


def test_entry_points_need_a_context():
    hexes = (C.c_char_p * 2)(PAY1.encode(), PAY2.encode())
    two = (C.c_void_p * 2)(None, None)
    h = C.c_void_p()
    calls = {
        "awm_add_mix_payloads_d": lambda: awm.lib.awm_add_mix_payloads_d(None, None, two, 2, 1024, 2, two, 0.01, 0, None, None, None, 0, 0),
        "awm_add_stream_create_payloads_at": lambda: awm.lib.awm_add_stream_create_payloads_at(None, bytes(16), hexes, 2, 2, 128, 0, C.byref(h)),
        "awm_add_watermark_payloads_file": lambda: awm.lib.awm_add_watermark_payloads_file(None, bytes(16), hexes, 2, b"in.wav", hexes, None, None),
        "awm_add_stream_watermark_payloads_file":
            lambda: awm.lib.awm_add_stream_watermark_payloads_file(None, bytes(16), hexes, 2, b"in.wav", hexes, None, None, 5000),
    }
    for what, call in calls.items():
        rc = call()
        assert rc < 0, what
        assert b"null context" in awm.lib.awm_last_error(), what
        with pytest.raises(awm.AwmError):
            binding._check(rc, what)
    assert not h.value


def test_null_stream_object():
    assert awm.lib.awm_add_stream_payloads(None) == 0
    p, k = (C.c_void_p * 6)(), (C.c_size_t * 3)()
    assert awm.lib.awm_add_stream_push_payloads(None, 0, 1, p, k) < 0
    assert b"bad argument" in awm.lib.awm_last_error()


def test_file_tile_hook():
    awm.set_payloads_file_tile(128)
    awm.set_payloads_file_tile(0)


def test_path_lists_are_checked_before_the_library_is_called(tmp_path):
    src = tmp_path / "in.wav"
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    assert binding.check_payload_paths([PAY1, PAY2], src, [a, str(b)]) == [os.fsencode(a), os.fsencode(b)]
    assert binding.check_payload_paths([], src, []) == []
    with pytest.raises(ValueError, match="2 payloads but 1 output paths"):
        binding.check_payload_paths([PAY1, PAY2], src, [a])
    with pytest.raises(ValueError, match=r"out_paths\[1\] equals out_paths\[0\]"):
        binding.check_payload_paths([PAY1, PAY2], src, [a, a])
    with pytest.raises(ValueError, match=r"out_paths\[1\] equals out_paths\[0\]"):
        binding.check_payload_paths([PAY1, PAY2], src, [a, tmp_path / "sub" / ".." / "a.wav"])       # the same path, spelled differently
    with pytest.raises(ValueError, match=r"out_paths\[1\] equals the input path"):
        binding.check_payload_paths([PAY1, PAY2], src, [a, src])
    with pytest.raises(TypeError, match=r"payloads\[0\]"):
        binding.check_payload_paths([b"00", PAY2], src, [a, b])
    with pytest.raises(TypeError, match="list of paths"):
        binding.check_payload_paths([PAY1], src, str(a))
    # Context.add_watermark_payloads_file runs the check first: no context is touched (there is none here)
    ctx = object.__new__(awm.Context)
    ctx._h = None
    with pytest.raises(ValueError):
        ctx.add_watermark_payloads_file(None, [PAY1, PAY2], src, [a, a])
    assert not a.exists()


def test_span_lists_are_checked_before_the_library_is_called():
    x = torch.zeros((2048, 2), dtype=torch.float32)
    outs = [torch.empty_like(x), torch.empty_like(x)]
    fm = [awm.tab_frame_mod(None, PAY1), awm.tab_frame_mod(None, PAY2)]
    bm = [torch.zeros(4), torch.zeros(4)]
    assert binding.check_mix_payloads(x, tuple(outs), fm, None) == (outs, fm, None)
    assert binding.check_mix_payloads(x, outs, fm, tuple(bm))[2] == bm
    with pytest.raises(ValueError, match="2 tables but 1 outputs"):
        binding.check_mix_payloads(x, outs[:1], fm, None)
    with pytest.raises(ValueError, match="2 outputs but 1 arrays"):
        binding.check_mix_payloads(x, outs, fm, bm[:1])
    with pytest.raises(ValueError, match="one length"):
        binding.check_mix_payloads(x, outs, fm, [bm[0], torch.zeros(5)])
    with pytest.raises(ValueError, match=r"outs\[1\]"):
        binding.check_mix_payloads(x, [outs[0], torch.empty((1024, 2))], fm, None)
    with pytest.raises(ValueError, match="pcm"):
        binding.check_mix_payloads(x.double(), outs, fm, None)


def test_tile_lists_are_checked_before_the_library_is_called():
    x = torch.zeros((2048, 2), dtype=torch.float32)
    ctx = object.__new__(awm.Context)
    ctx._h = None
    with pytest.raises(TypeError, match=r"payloads\[1\]"):
        ctx.add_watermark_payloads_tiles(None, [PAY1, 7], x)
    with pytest.raises(ValueError, match="pcm"):
        ctx.add_watermark_payloads_tiles(None, [PAY1, PAY2], x.double())
