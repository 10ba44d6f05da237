"""add_watermark_payloads without a GPU: the binding's argument checks raise before the library is called, and the entry point itself
refuses to run without a context (there is no CPU fallback)."""
import ctypes as C

import pytest
import torch

import audiowmark_amd as awm
from audiowmark_amd import binding

PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"


def test_output_list_is_checked_before_the_library_is_called():
    x = torch.zeros((2048, 2), dtype=torch.float32)
    ok = [torch.empty_like(x), torch.empty_like(x)]
    assert binding.check_payload_outputs([PAY1, PAY2], x, None) is None
    assert binding.check_payload_outputs([PAY1, PAY2], x, tuple(ok)) == ok
    with pytest.raises(ValueError, match="2 payloads but 1 outputs"):
        binding.check_payload_outputs([PAY1, PAY2], x, ok[:1])
    with pytest.raises(ValueError, match=r"outs\[1\]"):
        binding.check_payload_outputs([PAY1, PAY2], x, [ok[0], torch.empty_like(x, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"outs\[0\]"):
        binding.check_payload_outputs([PAY1, PAY2], x, [torch.empty((1024, 2)), ok[1]])
    with pytest.raises(ValueError, match=r"outs\[1\]"):
        binding.check_payload_outputs([PAY1, PAY2], x, [ok[0], torch.empty((2, 2048)).t()])       # not contiguous
    with pytest.raises(ValueError, match="pcm"):
        binding.check_payload_outputs([PAY1], x.double(), None)
    with pytest.raises(TypeError, match=r"payloads\[1\]"):
        binding.check_payload_outputs([PAY1, b"00"], x, None)


def test_entry_point_needs_a_context():
    """no context, no result: the call fails with an error text instead of computing anywhere else"""
    hexes = (C.c_char_p * 2)(PAY1.encode(), PAY2.encode())
    outs = (C.c_void_p * 2)(None, None)
    rc = awm.lib.awm_add_watermark_payloads_d(None, bytes(16), hexes, 2, None, outs, 1024, 2, 44100)
    assert rc < 0
    assert b"null context" in awm.lib.awm_last_error()
    with pytest.raises(awm.AwmError):
        binding._check(rc, "awm_add_watermark_payloads_d")


def test_toggle_and_tile_are_exported():
    assert awm.ADD_PAYLOADS_TILE >= 2
    assert awm.add_payloads_fused_in_use() in (0, 1)
    awm.set_add_payloads_fused(False)
    awm.set_add_payloads_fused(True)
