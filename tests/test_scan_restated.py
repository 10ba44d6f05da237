"""The numpy restatement of the approximate sync search (tests/_scan.py) pinned against the oracle and the compiled reference.
CPU only.  test_gpu_scan_edges.py holds awm_search_approx_d to this restatement bit for bit on the library's own dB rows, so it
is pinned here first, bit for bit as well and on every shape that file uses:
    search_approx (pcm) == restated scan + local mean over the rows of sync_fft (pcm)
once with both sides from the oracle and, where the reference is built, once with both sides from the reference.  The shapes
are small on purpose (a candidate costs 30 600 float additions in block mode, 61 200 in clip mode).  A case takes 1 - 3 s with
both sides: watermarking the material, four sync_fft and one search per side are most of it, the restatement about 0.2 - 0.4 s."""
import numpy as np
import pytest

import _oracle as orc
import _ref
import _scan
import audiowmark_amd as awm

KEY42 = awm.test_key(42)


def check(mod, key, pcm, clip):
    ch = pcm.shape[1]
    tab = mod.sync_bits(key, clip)
    assert np.array_equal(tab, orc.sync_bits(key, clip))
    _, S = _scan.counts(len(pcm), clip)
    planes = _scan.planes_of(lambda *a: mod.sync_fft(pcm, ch, *a), pcm, clip)
    idx, raw, mean = _scan.search_approx(tab, planes, S)
    widx, wraw, wmean = mod.search_approx(key, pcm, ch, clip)
    assert len(widx) == _scan.SHIFTS * S
    assert np.array_equal(idx, widx) and np.array_equal(raw, wraw) and np.array_equal(mean, wmean)
    return raw


def both(key, pcm, clip):
    raw = check(orc, key, pcm, clip)
    if _ref.available():
        check(_ref, key, pcm, clip)
    return raw


@pytest.mark.parametrize("case", _scan.BLOCK, ids=_scan.block_id)
def test_block_mode(case):
    key, pcm = _scan.block_pcm(case, KEY42)
    raw = both(key, pcm, False)
    assert len(raw) == 4 * case[0] and np.count_nonzero(raw) == len(raw)


@pytest.mark.parametrize("case", _scan.CLIP, ids=_scan.clip_id)
def test_clip_mode(case):
    pcm = _scan.clip_pcm(case)
    raw = both(None, pcm, True)
    assert len(raw) == 4 * 2240 and 2 * np.count_nonzero(raw) >= len(raw), np.count_nonzero(raw)      # no case passes by being empty


def test_the_run_ends_differ_per_shift():
    """the two clips with zeroed ends: the first / last frame that is transformed is not the same one in all four shifts"""
    for case in _scan.CLIP:
        if case[0] == "padded" and (case[3] or case[4]):
            pcm = _scan.clip_pcm(case)
            runs = [np.flatnonzero(have)[[0, -1]].tolist() for _, have in _scan.planes_of(lambda *a: orc.sync_fft(pcm, pcm.shape[1], *a), pcm, True)]
            assert len({r[0] for r in runs}) > 1 or len({r[1] for r in runs}) > 1, runs


def test_local_mean_and_silent_range_by_hand():
    raw = np.arange(60, dtype=np.float64) ** 2
    want = [np.mean([raw[i + j] for j in range(-20, 21) if abs(j) >= 4 and 0 <= i + j < 60]) for i in range(60)]
    assert np.allclose(_scan.local_mean(raw), want, rtol=1e-15, atol=0)
    assert np.array_equal(_scan.local_mean(raw[:3]), np.zeros(3))                  # no neighbour at distance 4: the mean stays 0
    x = np.zeros((10, 2), np.float32)
    assert _scan.silent_range(x, True) == (20, 20) and _scan.silent_range(x, False) == (0, 20)
    x[3, 1] = x[7, 0] = 1
    assert _scan.silent_range(x, True) == (7, 15)
