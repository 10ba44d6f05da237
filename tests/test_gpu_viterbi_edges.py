"""K8 (csrc/hip/viterbi.hip) held to conv_decode_soft where it is more than a plain add-compare-select: every input of
tests/golden/viterbi_edges.npz (tests/golden/make_viterbi_edges.py; test_viterbi_restated.py proves on the CPU what each of
them is good for) through awm_viterbi_decode in the decoder's three forms, bits and error values equal to the stored oracle
values exactly -- np.array_equal on the bits, the error values as float32 bit patterns with NaN equal to NaN.

    steered merges   a decision on the survivor path where old1 < old0 but the two chains of additions end equal: only the
                     repeat path ("risky") gives the low predecessor its tie; one in the checked rounds, in each third of the
                     12-step launch and in the single 4-step rounds
    exact ties       up to 128 on the survivor path; a decoder that hands them to the high predecessor returns other bits
    magnitudes       metrics of 1e7, differences of 1e-3, costs that overflow to +inf, -0.0 and denormals
    NaN and inf      a NaN anywhere but the first position (the block must take the checked path all the same), +-inf
    other lengths    every residue mod 4 from 15 steps (no payload bits at all) to 256 (64 rounds): each has a launch plan of its own

One call per (form, code type, length) with all inputs of the group as one batch, so finite and NaN blocks share launches."""
import ctypes as C
import os

import numpy as np
import pytest

import _viterbi as V

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = {"launch chain": (1, 0), "one launch": (1, 1), "one round per launch": (0, 0)}          # (viterbi_super, viterbi_persistent)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    ctx = awm.Context(0)
    yield awm, ctx
    ctx.close()


@pytest.fixture(scope="module")
def edges():
    return V.load_edges(os.path.join(HERE, "golden", "viterbi_edges.npz"))[0]


def forced(awm, form):
    class Forced:
        def __enter__(self):
            awm.lib.awm_debug_set_viterbi_super(FORMS[form][0])
            awm.lib.awm_debug_set_viterbi_persistent(FORMS[form][1])

        def __exit__(self, *exc):
            awm.lib.awm_debug_set_viterbi_super(1)
            awm.lib.awm_debug_set_viterbi_persistent(-1)
    return Forced()


@pytest.mark.parametrize("form", list(FORMS))
def test_every_fixture_input(gpu, edges, form):
    awm, ctx = gpu
    wrong = []
    with forced(awm, form):
        assert awm.lib.awm_debug_viterbi_one_launch_in_use() == FORMS[form][1]
        for (bt, n), items in sorted(edges.items()):
            soft = np.stack([x for _, x, _, _, _ in items])
            got_bits, got_err = ctx.viterbi_decode(bt, soft)
            assert got_bits.shape == (len(items), n - V.ORDER)
            for i, (name, _, bits, err, _) in enumerate(items):
                if not (np.array_equal(got_bits[i], bits) and V.same_float(got_err[i], err)):
                    wrong.append((V.TYPES[bt], n, name, int(np.count_nonzero(got_bits[i] != bits)), float(got_err[i]), float(err)))
    assert not wrong, wrong


def test_refusals(gpu, edges):
    """Lengths without a launch plan (fewer than the 15 termination steps, more than 64 rounds) and a coded length that is no
    multiple of the rate are refused on the host -- a negative code and a message, nothing launched, nothing written -- and the
    next valid call is as correct as ever."""
    awm, ctx = gpu
    lib = awm.lib
    for bt in (0, 2):
        R = V.rate(bt)
        for coded_len in [n * R for n in (0, 1, 2, 5, 14, 260)] + [143 * R + 1, 143 * R - 1, 20 * R + R // 2]:
            soft = np.full((2, coded_len), 0.25, np.float32)
            bits = np.full((2, 300), -7, np.int32)
            err = np.full(2, -7, np.float32)
            rc = lib.awm_viterbi_decode(ctx._h, bt, soft.ctypes.data_as(C.c_void_p), coded_len, 2, bits.ctypes.data_as(C.c_void_p),
                                        err.ctypes.data_as(C.c_void_p))
            assert rc < 0, (bt, coded_len, rc)
            assert b"viterbi" in lib.awm_last_error(), (bt, coded_len, lib.awm_last_error())
            assert (bits == -7).all() and (err == -7).all()
        items = edges[(bt, 143)]
        got_bits, got_err = ctx.viterbi_decode(bt, np.stack([x for _, x, _, _, _ in items]))
        assert np.array_equal(got_bits, np.stack([b for _, _, b, _, _ in items]))
        assert V.same_float(got_err, np.array([e for _, _, _, e, _ in items], np.float32))
    # an empty batch is no error
    assert lib.awm_viterbi_decode(ctx._h, 0, None, 858, 0, None, None) == 0
