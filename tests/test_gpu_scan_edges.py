"""The approximate sync search (K4 for four shifts + the streaming scan K5w + the local mean K5b behind awm_search_approx_d) held
BIT FOR BIT at the edges of K5w's tiles, through the C ABI only.

The scores of the search depend on the order of 12 x 2550 float additions per candidate, and a tolerance cannot see one term taken
from the wrong lane.  But both ends of the scan are exposed: awm_sync_fft_d runs the search's dB kernel for one shift and hands out
the rows and `have` flags that the search computes internally, awm_search_approx_d hands out the scores.  So, per case:
  1. the library's own (db, have) of the four shifts, through awm_sync_fft_d with the search's silent range;
  2. the reference's sync_decode on those rows for every start frame, and the local mean of the result -- tests/_scan.py, numpy in
     the reference's order of additions, pinned to the oracle and the compiled reference by test_scan_restated.py;
  3. awm_search_approx_d must return exactly these numbers (np.array_equal), at the indices start * 1024 + shift * 256.
Besides: the `have` flags are the oracle's, and the scores stay inside the suite's bars (5e-5 raw, 1e-5 mean, as test_search_approx)
of the oracle's search on the same PCM -- which holds the dB rows themselves, the only input step 3 takes on trust.

Step 1 and the search run the same per-frame arithmetic of K4 under two grid mappings (one stream | four interleaved streams): a
whole frame that differs between the two shows here as a mismatch of every candidate that reads it.

The shapes (tests/_scan.py, BLOCK and CLIP) are the smallest that sit on an edge of K5w: S = 1, the quad of a lane (3, 4, 5), the
tile of 252 candidates (251, 252, 253, 505), the XCD ranges (2017 = 8 x 252 + 1), the padded end of the matrix (n_db = 2240, 2241,
2304) and, in clip mode, runs of transformed frames whose ends cut through tiles and 64-frame chunks.  What they catch, by
inspection of a K5w broken on purpose (compiled, never run):
  * tiles advancing by 256 instead of 252: lane 63 has no lane above, so the candidates 253 .. 255 of every tile add 0 for the
    terms they take from it -- S = 505, 2017 and all of clip mode (from S = 254 on); 251, 252 and 253 stay clean;
  * a term of the upper lane added without the lane shift (alignment cases 1 - 3): the candidates 1 - 3 of every quad add the
    value four frames lower in 1, 2 or 3 of 4 sync frames -- every case but S = 1; 3, 4 and 5 with the fewest candidates around;
  * a wrong XCD range (per_xcd, the early return): tiles computed twice or never -- S = 2017 (per_xcd 2, 9 of 16 slots at work)
    and clip mode (9 tiles); S <= 252 runs one tile in slot 0 and cannot see it;
  * the loader's substitute for frames past the matrix taken a quad early: the frames n_db - 4 .. n_db - 1 become frame 0's and
    the last two candidates (13 + sync frame 2224 = 2237) read them -- S = 14 and 78, where the leading dimension is n_db itself;
    at S = 15 (n_db = 2241, one past a multiple of 64) the last frames lie in a chunk whose tail is padding;
  * clip mode, the last live sync frame of a chain dropped (fr < run1 taken one short) or the chunk range [c_lo, c_hi) one short:
    the first candidates of a tile lose the run's last frame, or a chain reads a chunk that never arrived -- the placed clips,
    whose run ends on, one before and behind a tile's first candidate (960, 1259, 1260, +-517 samples), and the zeroed ends.  (The
    other bound, fr + 255 >= run0, has three frames of slack by design: candidates 252 .. 255 of a tile are dropped);
  * clip mode, frame_bit_count from a run end that is one off: the weights of the six bits change for every candidate with a sync
    frame on that end -- every clip case."""
import numpy as np
import pytest

import _oracle as orc
import _scan

pytestmark = pytest.mark.gpu

RAW_TOL, MEAN_TOL = 5e-5, 1e-5             # the bars of test_gpu_parity.py::test_search_approx


@pytest.fixture(scope="module")
def gpu():
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    ctx = awm.Context(0)

    class G:
        pass
    g = G()
    g.torch, g.awm, g.ctx = torch, awm, ctx
    g.dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    yield g
    awm.lib.awm_debug_set_scan_generic(0)
    ctx.close()


def check(gpu, key, pcm, clip):
    ch = pcm.shape[1]
    n_db, S = _scan.counts(len(pcm), clip)
    x = gpu.dev(pcm)
    planes = [(db.cpu().numpy(), have.cpu().numpy()) for db, have in _scan.planes_of(lambda *a: gpu.ctx.sync_fft(x, *a), pcm, clip)]
    idx, raw, mean = _scan.search_approx(orc.sync_bits(key, clip), planes, S)
    gi, graw, gmean = gpu.ctx.search_approx(key, x, clip_mode=clip)
    print("S %d: %d of %d raw scores non-zero; raw %d mean %d of them differ from the restatement"
          % (S, np.count_nonzero(raw), raw.size, np.count_nonzero(graw != raw) if graw.shape == raw.shape else -1,
             np.count_nonzero(gmean != mean) if gmean.shape == mean.shape else -1))
    assert len(gi) == _scan.SHIFTS * S
    assert np.array_equal(gi, idx)
    assert np.array_equal(graw, raw), np.flatnonzero(graw != raw)[:32]
    assert np.array_equal(gmean, mean), np.flatnonzero(gmean != mean)[:32]
    assert 2 * np.count_nonzero(raw) >= raw.size                                  # no case passes by being empty
    # the rows themselves: the oracle's flags, and scores inside the suite's bars of the oracle's search on the PCM
    for (_, have), (_, want_have) in zip(planes, _scan.planes_of(lambda *a: orc.sync_fft(pcm, ch, *a), pcm, clip)):
        assert np.array_equal(have, want_have)
    oi, oraw, omean = orc.search_approx(key, pcm, ch, clip)
    print("against the oracle: raw %.3g mean %.3g" % (np.abs(graw - oraw).max(), np.abs(gmean - omean).max()))
    assert np.array_equal(gi, oi)
    assert np.abs(graw - oraw).max() < RAW_TOL and np.abs(gmean - omean).max() < MEAN_TOL


@pytest.mark.parametrize("case", _scan.BLOCK, ids=_scan.block_id)
def test_block_mode(gpu, case):
    key, pcm = _scan.block_pcm(case, gpu.awm.test_key(42))
    check(gpu, key, pcm, False)


@pytest.mark.parametrize("case", _scan.CLIP, ids=_scan.clip_id)
def test_clip_mode(gpu, case):
    check(gpu, None, _scan.clip_pcm(case), True)


GENERIC = ([pytest.param(False, _scan.BLOCK[i], id=_scan.block_id(_scan.BLOCK[i])) for i in (0, 6, 9)]
           + [pytest.param(True, _scan.CLIP[i], id=_scan.clip_id(_scan.CLIP[i])) for i in (0, 6, 9)])


def run_case(gpu, clip, case):
    if clip:
        check(gpu, None, _scan.clip_pcm(case), True)
    else:
        key, pcm = _scan.block_pcm(case, gpu.awm.test_key(42))
        check(gpu, key, pcm, False)


@pytest.mark.parametrize("clip,case", GENERIC)
def test_generic_fallback(gpu, clip, case):
    """launch_sync_scan_window's fallback, the generic K5 (one lane per candidate, tiles of 64), is reachable in production and holds
    to the same numbers.  The scores cannot tell which kernel ran, so the library counts the launches that took the fallback: one
    per search with the switch on, none with it off"""
    launches = gpu.awm.lib.awm_debug_scan_generic_launches
    before = launches()
    gpu.awm.lib.awm_debug_set_scan_generic(1)
    try:
        run_case(gpu, clip, case)
    finally:
        gpu.awm.lib.awm_debug_set_scan_generic(0)
    assert launches() == before + 1


def test_streaming_kernel_by_default(gpu):
    """without the switch the shapes of this file go through K5w, not through the fallback"""
    launches = gpu.awm.lib.awm_debug_scan_generic_launches
    before = launches()
    run_case(gpu, False, _scan.BLOCK[1])
    run_case(gpu, True, _scan.CLIP[0])
    assert launches() == before
