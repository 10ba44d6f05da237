"""add_watermark_payloads at other sample rates without a GPU: the switch and the query of the path are exported, the profiling id of K10m
is there under the kernel's name, and the entry point still refuses to run without a context at 48 kHz (there is no CPU fallback)."""
import ctypes as C

import audiowmark_amd as awm

PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"


def test_switch_and_query_are_exported():
    assert awm.add_payloads_rate_fused_in_use() in (0, 1, 2)
    for mode in (0, 1, 2):
        awm.set_add_payloads_rate_fused(mode)
    assert awm.add_payloads_fused_in_use() in (0, 1)


def test_profiling_id_of_the_new_kernel():
    awm.lib.awm_prof_name.restype = C.c_char_p
    names = [awm.lib.awm_prof_name(i).decode() for i in range(awm.lib.awm_prof_count())]
    assert names.count("resample_mix_multi_kernel") == 1
    assert "resample_kernel" in names and "add_mix_multi_kernel" in names and all(names)


def test_entry_point_needs_a_context_at_48_khz():
    hexes = (C.c_char_p * 2)(PAY1.encode(), PAY2.encode())
    outs = (C.c_void_p * 2)(None, None)
    rc = awm.lib.awm_add_watermark_payloads_d(None, bytes(16), hexes, 2, None, outs, 1024, 2, 48000)
    assert rc < 0
    assert b"null context" in awm.lib.awm_last_error()
