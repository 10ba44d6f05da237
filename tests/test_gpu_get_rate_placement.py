"""`get` at 48 kHz on clips that are only 4-byte aligned, between NaN guards (tests/_placement.Arena): the input of K10c needs the
alignment of a float and nothing outside [pointer, pointer + size) is read.  A read past either end would bring a NaN into the taps and
show in the slices' bits and in the patterns, which are compared with those of the same clips at aligned placements; 4- and 12-byte
offsets take the generic taps for stereo, 0 and 8 the phase form -- all forms give identical bits."""
import numpy as np
import pytest

import _placement as P

pytestmark = pytest.mark.gpu

PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"
R48 = 48000
OFFSETS = (0, 4, 8, 12)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"

    class G:
        pass
    g = G()
    g.torch, g.awm, g.ctx = torch, awm, awm.Context(0)
    g.arena = lambda *nbytes: P.Arena(torch, P.need(*nbytes), device="cuda")
    yield g
    awm.set_params()


def clips_48k(gpu, ch, secs):
    """marked and plain clips at 48 kHz as numpy arrays; the first ends in silence, the second begins with it"""
    t = gpu.torch
    out = []
    for i, s in enumerate(secs):
        gen = t.Generator(device="cuda")
        gen.manual_seed(3100 + 10 * ch + i)
        n = int(s * R48) + 7 * i + 1
        x = (t.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=t.float32) * 2 - 1).contiguous()
        if s >= 20:
            x = gpu.ctx.add_watermark(None, PAY1 if i % 2 else PAY2, x, sample_rate=R48)
        if i == 0:
            x[n - n // 6:] = 0
        if i == 1:
            x[: n // 7] = 0
        out.append(x.cpu().numpy())
    return out


@pytest.mark.parametrize("ch,secs", [(2, (22, 3.1, 25, 0.05, 4.7, 30)), (1, (24, 2.9, 0.04, 5.3))], ids=["stereo", "mono"])
def test_misaligned_clips(gpu, ch, secs):
    t = gpu.torch
    clips = clips_48k(gpu, ch, secs)
    dev = [t.from_numpy(c).cuda() for c in clips]
    aligned = gpu.ctx.get_watermark_batch(None, dev, sample_rate=R48)
    aligned_slices, aligned_ranges = gpu.ctx.clip_stage(dev, R48)
    assert any(aligned) and all(r[1] > r[0] >= 0 for r in aligned_ranges)
    for shift in range(len(OFFSETS)):
        offsets = [OFFSETS[(i + shift) % len(OFFSETS)] for i in range(len(clips))]
        a = gpu.arena(*[c.nbytes for c in clips])
        placed = [a.place(c, t.float32, o, name="clip %d" % i) for i, (c, o) in enumerate(zip(clips, offsets))]
        assert [p.data_ptr() % 16 for p in placed] == offsets
        assert gpu.ctx.get_watermark_batch(None, placed, sample_rate=R48) == aligned
        slices, ranges = gpu.ctx.clip_stage(placed, R48)
        assert t.equal(slices.view(t.int32), aligned_slices.view(t.int32))
        assert np.array_equal(ranges, aligned_ranges)
        a.check()
