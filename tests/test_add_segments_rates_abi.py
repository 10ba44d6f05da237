"""The segment batches with a sample rate per segment, as far as they can be checked without a device: the header
declares the four entry points, the library exports them with the argument types the binding declares, and the binding's wrappers refuse
a rate sequence of the wrong length before anything is called."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["awm_add_watermark_segments_rates_d", "awm_add_watermark_segments_keys_rates_d", "awm_add_watermark_segments_rates_s16_d",
         "awm_add_watermark_segments_keys_rates_s16_d"]


def test_the_header_declares_the_four_entry_points():
    with open(os.path.join(ROOT, "include", "awm_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        m = re.search(r"\bint " + name + r" \(([^;]*)\);", header)
        assert m, name + " is not declared"
        args = " ".join(m.group(1).split())
        assert args.endswith("int n_channels, const int *sample_rates"), name + ": " + args
        sample = "int16_t" if "s16" in name else "float"
        assert "const %s *const *pcm_in_d, %s *const *out_d" % (sample, sample) in args
    assert "Not offered: the command line, the file level, the tile stream, the awm_multi_* / sharded forms" in header


def test_the_library_exports_them_and_the_binding_declares_them():
    import audiowmark_amd as awm
    raw = C.CDLL(awm.binding.library_path())
    for name in NAMES:
        assert hasattr(raw, name), name + " is not exported"
        argtypes = getattr(awm.lib, name).argtypes
        assert argtypes is not None and len(argtypes) == 10 and argtypes[8] is C.c_int and argtypes[9] is C.c_void_p


def test_a_rate_sequence_of_the_wrong_length_is_refused_before_any_call():
    import torch
    import audiowmark_amd as awm
    segs = [torch.zeros((8, 2)), torch.zeros((8, 2))]
    segs16 = [torch.zeros((8, 2), dtype=torch.int16)] * 2
    pays = ["00" * 16] * 2

    class NoContext:                                        # (any use of the context's handle would raise AttributeError)
        pass
    for rates in ([48000], [48000, 32000, 44100], []):
        with pytest.raises(ValueError, match="%d rates for 2" % len(rates)):
            awm.Context.add_watermark_segments(NoContext(), None, pays, segs, [0, 0], sample_rate=rates)
        with pytest.raises(ValueError, match="%d rates for 2" % len(rates)):
            awm.Context.add_watermark_segments_keys(NoContext(), [None, None], pays, segs, [0, 0], sample_rate=rates)
        with pytest.raises(ValueError, match="%d rates for 2" % len(rates)):
            awm.Context.add_watermark_segments_s16(NoContext(), None, pays, segs16, [0, 0], sample_rate=rates)
        with pytest.raises(ValueError, match="%d rates for 2" % len(rates)):
            awm.Context.add_watermark_segments_keys_s16(NoContext(), [None, None], pays, segs16, [0, 0], sample_rate=rates)
