"""The limiter of every `add` path on material with real dynamics: block maxima (taken inside the mix kernels K2, K2m, the batch form
of K2, and K11 for other sample rates) and the gain ramp between neighbouring blocks (K3: table + float4 apply, the scalar generic
form, the batch form), against the numpy restatement of the reference's limiter (tests/_limiter.py, pinned to the oracle and the
compiled reference bit for bit by test_limiter_restated.py).

Two assertions throughout:
  (A) self-consistency, BIT FOR BIT: the entry point's output with the limiter == np_limiter (the same entry point's output with
      test_no_limiter).  No tolerance: the kernels round every operation on its own (__fdiv_rn / __fmul_rn / __fadd_rn), as the
      restatement does.  A ramp index that is one sample off changes the output by 7e-7 at most on the ladder material -- under
      the bars of (B), so this is the assertion that finds it.
  (B) against the oracle's `add` of the same input, with the project's bars for `add` (test_gpu_parity.py: RMS 1e-6, max 2e-6).

The materials (tests/_limiter.py): "dynamics" D -- single loud samples at the first / last sample of a block, blocks under the ceiling
whose ramp is the identity (K3 skips such runs) next to blocks that ramp, a block just over the ceiling, the stream's maximum on its
very last sample in a partial block; "ladder" L -- 17 blocks with strictly rising peaks on both sides of every block boundary: a
boundary sample counted in the neighbouring block changes a block maximum by 0.02.  Boundaries 14 and 15 lie at offsets 952 and 1020
of a 1024 sample frame, in the 128 sample tail that K2 stores one frame later; boundary 16 wraps to offset 64.

What the module notices was tried on deliberately wrong builds of the kernels (arithmetic only), all cases pass on the real ones:
  K2's tail path with `x <= pbound`                       -> every L case through K2 (boundaries 14, 15), no D case
  K2m's body with `x <= bound` / its tail with `<=`       -> the payloads cases (the tail: L alone)
  K11 with `v <= bound`                                   -> every case at another rate (stereo too: L's peak behind a boundary is in channel 0)
  K3's apply kernel skipping on its first entry alone     -> D at 1, 2 channels, test_ramp_alone aligned
  ramp index + 1 in the scalar kernel / behind a boundary inside a run of the apply kernel / in the batch remainder
                                                          -> 3 channels and unaligned spans / every 1, 2 channel case / the batches
Measured against the oracle (B): RMS <= 9.8e-10, max <= 6.0e-8 over all cases.

Not reached: at 44100 Hz every boundary lies on an even offset inside a frame (44100 k mod 1024 is even), and K2 handles sample
pairs (2 lane, 2 lane + 1) -- the case that a pair is split by a boundary (`x + 1 < bound` false where `x < bound` is true) cannot
occur through the public entries, which fix the block at 44100 samples for this kernel."""
import numpy as np
import pytest

import _limiter as lim
import _oracle as orc

pytestmark = pytest.mark.gpu

PAY1 = "0123456789abcdef0011223344556677"
RMS_TOL = 1e-6          # the project's bars for `add` against the oracle (test_gpu_parity.py)
MAX_TOL = 2e-6
BS = 44100
TILE = 128              # frames of 1024 samples: the smallest tile of add_watermark_tiles


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

    def dev(a):
        a = np.ascontiguousarray(a, np.float32)
        return torch.from_numpy(a[:, 0] if a.ndim == 2 and a.shape[1] == 1 else a).cuda()      # mono: [frames], as the other modules pass it
    g.dev = dev
    g.host = lambda t: t.cpu().numpy().reshape(t.shape[0], -1)
    yield g
    awm.set_params()
    orc.set_params()
    ctx.close()


def material(name, ch, block=BS, frames=None):
    x = lim.dynamics(ch, block) if name == "D" else lim.ladder(17, ch, block)
    return x if frames is None else np.ascontiguousarray(x[:frames])


def same_bits(got, want, what=""):
    got, want = lim.bits(got).reshape(-1), lim.bits(want).reshape(-1)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} values differ, the first at value index {bad[0]}"


def both(gpu, fn):
    """(without limiter, with limiter) of fn (): the same entry point under test_no_limiter and under the defaults"""
    gpu.awm.set_params(test_no_limiter=True)
    try:
        mix = fn()
    finally:
        gpu.awm.set_params()
    return mix, fn()


def check_a(gpu, mix, limited, block=BS, zero_frames=0, what=""):
    want, _ = lim.np_limiter(gpu.host(mix), block, zero_frames=zero_frames)
    same_bits(gpu.host(limited), want, what + " (A: limiter on == np_limiter of the same path's mix)")


def check_b(gpu, limited, x, ch, rate=BS, what=""):
    want = orc.add(None, x, ch, PAY1, rate).reshape(len(x), ch)
    d = gpu.host(limited).astype(np.float64) - want
    r, m = float(np.sqrt((d * d).mean())), float(np.abs(d).max())
    print(f"{what}: against the oracle rms {r:.3e} max {m:.3e}")
    assert r < RMS_TOL and m < MAX_TOL, (what, r, m)


# ---- 1. block maxima of K2, directly; 2. the same through spans -----------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(gpu):
    """(name, ch) -> (input on the device, mix, block maxima, limited) of ONE launch of K2 over the whole stream + K3, as numpy;
    computed once, shared by the cases below and left unchanged"""
    cache = {}

    def get(name, ch):
        if (name, ch) not in cache:
            t = gpu.torch
            x = gpu.dev(material(name, ch))
            n = x.shape[0]
            fm = gpu.awm.tab_frame_mod(None, PAY1)
            bm = t.empty(n // BS + 3, dtype=t.float32, device="cuda")
            gpu.ctx.add_init_block_max(bm)
            out = t.empty_like(x)
            gpu.ctx.add_mix(x, out, fm, 0.01, 0, None, None, bm)
            mix = gpu.host(out).copy()
            gpu.ctx.add_limit(out, 0, bm)
            cache[name, ch] = (x, fm, mix, bm.cpu().numpy(), gpu.host(out).copy())
        return cache[name, ch]
    return get


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("name", ["D", "L"])
def test_block_maxima_and_ramp_of_one_launch(gpu, whole, name, ch):
    x, _, mix, bm, limited = whole(name, ch)
    n = len(mix)
    n_blocks = -(-n // BS)
    want = lim.block_maxima(mix, BS)
    assert len(want) == n_blocks < len(bm)
    same_bits(bm[:n_blocks], want, "block maxima")                         # == max (0.99, max |mix| in block k), exactly
    same_bits(bm[n_blocks:], np.full(len(bm) - n_blocks, lim.CEILING), "entries behind the stream's last block")
    same_bits(limited, lim.np_limiter(mix, BS)[0], "add_limit on add_mix's output")
    if name == "L":                                                        # the ladder is still one with the watermark in it
        assert np.all(np.diff(want) > 0.01)
    # the mix of this entry is the mix of add_watermark
    gpu.awm.set_params(test_no_limiter=True)
    try:
        same_bits(gpu.host(gpu.ctx.add_watermark(None, PAY1, x)), mix, "add_watermark without limiter")
    finally:
        gpu.awm.set_params()


def span_cuts(name):
    """cuts on frame boundaries: frame 47 (sample 48128, inside block 1); frames next to the one whose 128 sample tail holds a block
    boundary (L: boundary 14 = frame 602 + 952, boundary 15 = frame 645 + 1020; D: its peaks at 3 BS - 1 and 6 BS)"""
    if name == "L":
        assert 14 * BS == 602 * 1024 + 952 and 15 * BS == 645 * 1024 + 1020
        return [(47,), (47, 603), (602, 646), (603, 645)]
    return [(47,), (47, 130), (129, 259)]


@pytest.mark.parametrize("windows", [False, True], ids=["shared_table", "window_per_span"])
@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("name", ["D", "L"])
def test_spans_equal_one_launch(gpu, whole, name, ch, windows):
    """two and three spans with halo frames (as test_add_sharded_spans_equal_whole): block maxima into one shared table, or into a
    window of its own per span (first_block != 0) that is max-reduced afterwards, as sharded ranks do; add_limit per span"""
    t = gpu.torch
    x, fm, mix, bm_whole, limited = whole(name, ch)
    n = x.shape[0]
    for cuts in span_cuts(name):
        edges = [0] + [c * 1024 for c in cuts] + [n]
        assert all(a < b for a, b in zip(edges, edges[1:])) and edges[-2] + 2048 < n
        out = t.empty_like(x)
        bm = t.empty(len(bm_whole), dtype=t.float32, device="cuda")
        gpu.ctx.add_init_block_max(bm)
        for a, b in zip(edges, edges[1:]):
            before = x[a - 1024:a].contiguous() if a else None
            after = x[b:b + 1024].contiguous() if b < n else None
            if windows:
                fb = a // BS
                win = t.empty((b - 1) // BS - fb + 1, dtype=t.float32, device="cuda")
                gpu.ctx.add_init_block_max(win)
                gpu.ctx.add_mix(x[a:b], out[a:b], fm, 0.01, a // 1024, before, after, win, first_block=fb)
                bm[fb:fb + len(win)] = t.maximum(bm[fb:fb + len(win)], win)
            else:
                gpu.ctx.add_mix(x[a:b], out[a:b], fm, 0.01, a // 1024, before, after, bm)
        same_bits(gpu.host(out), mix, f"mix of spans {cuts}")
        same_bits(bm.cpu().numpy(), bm_whole, f"block maxima of spans {cuts}")
        for a, b in zip(edges, edges[1:]):
            gpu.ctx.add_limit(out[a:b], a, bm)
        same_bits(gpu.host(out), limited, f"limited spans {cuts}")


@pytest.mark.parametrize("ch,pair", [(1, 1), (2, 1), (2, 0), (3, 1)], ids=["mono", "stereo_paired", "stereo_unpaired", "three_channels"])
def test_span_with_a_block_in_front_of_its_maxima(gpu, ch, pair):
    """every instantiation of K2 (a channel per wave; stereo with the paired and with the single transforms) on ONE span through
    awm_add_mix_d: first_frame 3, both halos, first_block 1 -- the maximum of block 0 falls in front of the array and is dropped --, and
    43 frames + 1000 samples: a ragged last frame, and the block boundary 44100 = frame 43 + 68 inside a frame (bounded stores, two running
    maxima) and, one frame later, in front of that frame's tail.  The maxima against the numpy restatement on the returned mix, the mix
    against the whole-stream launch over the enclosing stream (whose samples behind the ragged frame's 1000 are silence up to the halo)"""
    t = gpu.torch
    first, n = 3 * 1024, 43 * 1024 + 1000
    end, halo = first + n, 47 * 1024
    assert first < BS < end < halo and halo - end == 24
    x = np.random.default_rng(40 + ch).uniform(-1, 1, (50 * 1024, ch)).astype(np.float32)
    x[:BS] *= 1.5                         # block 0 is the louder one: its maximum stored at index 0 instead of dropped would show
    x[BS:] *= 1.2
    x[end:halo] = 0
    xd = gpu.dev(x)
    fm = gpu.awm.tab_frame_mod(None, PAY1)
    out_whole, out = t.empty_like(xd), t.empty_like(xd[first:end])
    bm = t.empty(2, dtype=t.float32, device="cuda")
    gpu.ctx.add_init_block_max(bm)
    gpu.awm.lib.awm_debug_set_fft_pair(pair)
    try:
        gpu.ctx.add_mix(xd, out_whole, fm, 0.01, 0, None, None, None)
        gpu.ctx.add_mix(xd[first:end], out, fm, 0.01, 3, xd[first - 1024:first].contiguous(), xd[halo:halo + 1024].contiguous(), bm, first_block=1)
        mix = gpu.host(out)
        same_bits(mix, gpu.host(out_whole)[first:end], "mix of the span against the whole-stream launch")
    finally:
        gpu.awm.lib.awm_debug_set_fft_pair(1)
    in_block_0, in_block_1 = lim.block_maxima(mix[:BS - first], BS), lim.block_maxima(mix[BS - first:], BS)
    assert len(in_block_0) == len(in_block_1) == 1 and in_block_0[0] > in_block_1[0] > lim.CEILING
    same_bits(bm.cpu().numpy(), np.array([in_block_1[0], lim.CEILING], np.float32), "block maxima from block 1 on")


# ---- 3. K3 alone, with hand-made block maxima -------------------------------------------------------------------------------------
# entries under the ceiling count as the ceiling; blocks 2 - 4 are under it: the ramp of block 3 is the identity (K3 skips its runs), those
# of 2 and 4 are not; with the window that begins at block 2, blocks 0 - 3 are the identity
TABLE = np.array([0.5, 2.0, 0.99, 0.3, 0.7, 1.7, 1.0, 0.25, 3.0, 1.25], np.float32)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "one_float_in"])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_ramp_alone(gpu, ch, aligned):
    """add_limit on arbitrary data: spans that begin anywhere in a block, lengths under one float4 / one run of the apply kernel /
    several runs with a remainder / more than two blocks; a 16 byte aligned span (1, 2 channels: table + float4 apply kernel + scalar
    remainder) and one that starts one float into the allocation (the scalar kernel for everything); a table that begins at block 0
    and a window of it that begins at block 2.  Nothing outside the span is written."""
    t = gpu.torch
    rng = np.random.default_rng(40 + ch)
    guard, off = 777.25, (4 if aligned else 5)
    table = gpu.dev(TABLE)
    for n in (1, 3, 8191, 8192 * 4 + 3, 2 * BS + 1):
        data = rng.uniform(-2, 2, (n, ch)).astype(np.float32)
        for first in (0, 1, 1021, 44099, 44100, 3 * 44100 + 5):
            for fb in (0, 2):
                buf = t.full((n * ch + 16,), guard, dtype=t.float32, device="cuda")
                span = buf[off:off + n * ch]
                span.copy_(t.from_numpy(data.reshape(-1)).cuda())
                view = span if ch == 1 else span.view(n, ch)
                assert (view.data_ptr() % 16 == 0) == aligned
                gpu.ctx.add_limit(view, first, table[fb:], first_block=fb)
                got = buf.cpu().numpy()
                what = f"n {n} first_sample {first} first_block {fb}"
                same_bits(got[off:off + n * ch], lim.ramp(data, first, TABLE[fb:], BS, first_block=fb), what)
                assert np.all(got[:off] == guard) and np.all(got[off + n * ch:] == guard), what + ": written outside the span"


# ---- 4. add_watermark ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ch", [("D", 1), ("D", 2), ("D", 3), ("L", 2)])
def test_add_watermark(gpu, name, ch):
    x = material(name, ch)
    xd = gpu.dev(x)
    mix, limited = both(gpu, lambda: gpu.ctx.add_watermark(None, PAY1, xd))
    check_a(gpu, mix, limited, what=f"{name} ch {ch}")
    check_b(gpu, limited, x, ch, what=f"{name} ch {ch}")


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("n", [1, BS - 1, BS, BS + 1, 2 * BS], ids=["1", "BS-1", "BS", "BS+1", "2BS"])
def test_add_watermark_edge_lengths(gpu, n, ch):
    """the stream's maximum (2.5) on its last sample: alone in the stream, at the end of a partial / a whole block, in a last block
    of ONE sample (BS + 1), at the end of the second block"""
    x = lim.peak_at_end(n, ch)
    xd = gpu.dev(x)
    mix, limited = both(gpu, lambda: gpu.ctx.add_watermark(None, PAY1, xd))
    check_a(gpu, mix, limited, what=f"n {n} ch {ch}")
    check_b(gpu, limited, x, ch, what=f"n {n} ch {ch}")
    assert np.abs(gpu.host(limited)).max() <= np.nextafter(lim.CEILING, np.float32(1))


# ---- 5. add_watermark_payloads (K2m) ------------------------------------------------------------------------------------------------
def five_payloads():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, 16, dtype=np.uint8).tobytes().hex() for _ in range(5)]


@pytest.mark.parametrize("name,ch", [("D", 2), ("D", 1), ("L", 2), ("D", 3)])
def test_add_watermark_payloads(gpu, name, ch):
    """five payloads: two tile passes of the fused kernel, block maxima and ramp per output"""
    assert 1 <= gpu.awm.ADD_PAYLOADS_TILE < 5
    xd = gpu.dev(material(name, ch))
    pays = five_payloads()
    mixes, outs = both(gpu, lambda: gpu.ctx.add_watermark_payloads(None, pays, xd))
    assert gpu.awm.add_payloads_fused_in_use() == 1
    for p, pay in enumerate(pays):
        check_a(gpu, mixes[p], outs[p], what=f"{name} ch {ch} output {p}")
        assert gpu.torch.equal(outs[p], gpu.ctx.add_watermark(None, pay, xd)), f"output {p} differs from add_watermark"
    assert not gpu.torch.equal(outs[0], outs[4])


# ---- 6. batches of clips ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", [False, True], ids=["add_watermark_batch", "add_watermark_batch_keys"])
def test_batches(gpu, keys):
    """one batch of stereo clips cut from D and L: shorter than a block, a block, a last block of one sample, two blocks and a sample,
    the whole material -- block maxima and ramp tables per clip"""
    D, L = material("D", 2), material("L", 2)
    clips = [gpu.dev(m[:n]) for m in (D, L) for n in (BS - 5, BS, BS + 1, 2 * BS + 1, len(m))]
    if keys:
        ks = [gpu.awm.test_key(100 + i) for i in range(len(clips))]
        run = lambda: gpu.ctx.add_watermark_batch_keys(ks, PAY1, clips)
    else:
        ks = [None] * len(clips)
        run = lambda: gpu.ctx.add_watermark_batch(None, PAY1, clips)
    mixes, outs = both(gpu, run)
    for i, c in enumerate(clips):
        check_a(gpu, mixes[i], outs[i], what=f"clip {i} of {c.shape[0]} frames")
        assert gpu.torch.equal(outs[i], gpu.ctx.add_watermark(ks[i], PAY1, c)), f"clip {i} differs from add_watermark"


# ---- 7. the tile loop, streams that start inside the grid ---------------------------------------------------------------------------
@pytest.mark.parametrize("zero_frames", [0, 1, 44099, 3 * 1024 + 17])
@pytest.mark.parametrize("name", ["L", "D"])
def test_add_watermark_tiles(gpu, name, zero_frames):
    """the stream begins zero_frames samples into the frame / block grid: the material is cut so that its peaks lie on the boundaries
    of THAT grid (the material with its first zero_frames samples silenced is what the limiter sees)"""
    t = gpu.torch
    xd = gpu.dev(material(name, 2)[zero_frames:])
    mix, limited = both(gpu, lambda: gpu.ctx.add_watermark_tiles(None, PAY1, xd, TILE, zero_frames=zero_frames))
    check_a(gpu, mix, limited, zero_frames=zero_frames, what=f"{name} zero_frames {zero_frames}")
    zx = t.cat([t.zeros((zero_frames, 2), device="cuda"), xd])
    assert t.equal(limited, gpu.ctx.add_watermark(None, PAY1, zx)[zero_frames:])


# ---- 8. other sample rates: K11 takes the maxima, the block is one second of that rate ----------------------------------------------
@pytest.mark.parametrize("name", ["D", "L"])
@pytest.mark.parametrize("rate,ch", [(48000, 2), (11025, 1), (8000, 2)])
def test_other_rates(gpu, rate, ch, name):
    """48000 Hz stereo; 11025 Hz mono (block >= 8192: the table + float4 apply kernels); 8000 Hz stereo (block < 8192: the scalar
    kernel; K11 with a block that is shorter than some of its runs' reach)"""
    x = material(name, ch, rate)
    xd = gpu.dev(x)
    mix, limited = both(gpu, lambda: gpu.ctx.add_watermark(None, PAY1, xd, sample_rate=rate))
    check_a(gpu, mix, limited, block=rate, what=f"{name} {rate} Hz ch {ch}")
    check_b(gpu, limited, x, ch, rate, what=f"{name} {rate} Hz ch {ch}")
