"""K10s, the phase-per-thread resamplers for a span of a stream (awm_debug_resample_span_d), against the same outputs
of awm_resample_d on the whole stream, bit for bit (torch.equal), 48 -> 44.1 kHz and 44.1 -> 48 kHz.

A span begins on a multiple of np and is given the part of the stream that is resident; everything else reads as zero.  The spans are the
ones where the index arithmetic can go wrong: the first tile, a start inside a tile of the kernel (R J np = 16 np outputs), on its edge
and thousands of tiles in, lengths of one output, less than a group, a tile +- 1 and several tiles and a bit, a resident range that cuts
the first and the last window, and a start near 2^40 with nothing but the window resident.  The whole-stream results are computed once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_IN = 10_600_000                     # enough for a span that begins 4097 tiles in, in either direction
GUARD = 64
DIRECTIONS = {"down": (48000, 44100, 147, 160, 18), "up": (44100, 48000, 160, 147, 16)}       # rate_in, rate_out, np, step, hl

_CACHE = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    ctx = awm.Context(0)
    awm.lib.awm_debug_set_resample_phase(1)

    class G:
        pass
    g = G()
    g.torch, g.awm, g.ctx = torch, awm, ctx

    def stream(ch=2, n=N_IN, seed=5):
        if ("x", ch, n, seed) not in _CACHE:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed)
            x = torch.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1
            _CACHE[("x", ch, n, seed)] = x.contiguous()
        return _CACHE[("x", ch, n, seed)]
    g.stream = stream

    def whole(direction, ch=2, n=N_IN, seed=5):
        rate_in, rate_out = DIRECTIONS[direction][:2]
        if ("y", direction, ch, n, seed) not in _CACHE:
            _CACHE[("y", direction, ch, n, seed)] = ctx.resample(stream(ch, n, seed), rate_in, rate_out)
            ctx.synchronize()
        return _CACHE[("y", direction, ch, n, seed)]
    g.whole = whole
    yield g
    _CACHE.clear()
    awm.lib.awm_debug_set_resample_phase(1)
    ctx.close()


def span(gpu, direction, resident, in0, out0, n_out, shift=0):
    """the span between guard values -> (outputs, phase_form_used); shift: floats the output is moved off the 8-byte grid"""
    t = gpu.torch
    rate_in, rate_out = DIRECTIONS[direction][:2]
    ch = resident.shape[1] if resident.dim() > 1 else 1
    room = t.full((2 * GUARD + n_out * ch + 2,), float("nan"), dtype=t.float32, device="cuda")
    out = room[GUARD + shift:GUARD + shift + n_out * ch]
    out = out.view(n_out, ch) if ch > 1 else out
    _, used = gpu.ctx.resample_span(resident, in0, out0, n_out, rate_in, rate_out, out=out)
    gpu.ctx.synchronize()
    assert bool(t.isnan(room[:GUARD + shift]).all()) and bool(t.isnan(room[GUARD + shift + n_out * ch:]).all()), "a guard value was overwritten"
    return out, used


@pytest.mark.parametrize("direction", ["down", "up"])
def test_spans_of_a_resident_stream(gpu, direction):
    np_ = DIRECTIONS[direction][2]
    x, y = gpu.stream(), gpu.whole(direction)
    for out0 in (0, np_, 15 * np_, 16 * np_, 16 * np_ * 4097):
        for n_out in (1, np_ - 1, 16 * np_ - 1, 16 * np_ + 1, 5 * 16 * np_ + 7):
            assert out0 + n_out <= y.shape[0]
            got, used = span(gpu, direction, x, 0, out0, n_out)
            assert used == 1, (out0, n_out)
            assert gpu.torch.equal(got, y[out0:out0 + n_out]), (direction, out0, n_out)


@pytest.mark.parametrize("direction", ["down", "up"])
def test_resident_range_that_cuts_the_first_and_the_last_window(gpu, direction):
    """the samples outside the resident range read as zero: the expected values are those of the stream with zeros there"""
    t = gpu.torch
    _, _, np_, step, hl = DIRECTIONS[direction]
    out0, n_out = 16 * np_ * 3 + 5 * np_, 2 * 16 * np_ + 9
    first = out0 * step // np_ - hl + 1                      # the windows of the span: first .. last
    last = (out0 + n_out - 1) * step // np_ + hl
    a, b = first + hl, last - hl + 1                          # resident: a .. b - 1, half a window short on either side
    n = last + 1000
    x = gpu.stream()[:n]
    cut = t.zeros_like(x)
    cut[a:b] = x[a:b]
    y = gpu.ctx.resample(cut, *DIRECTIONS[direction][:2])
    got, used = span(gpu, direction, x[a:b].contiguous(), a, out0, n_out)
    assert used == 1
    assert t.equal(got, y[out0:out0 + n_out])
    full, _ = span(gpu, direction, x, 0, out0, n_out)
    assert not t.equal(got, full)                             # (the cut does reach the windows)


@pytest.mark.parametrize("direction", ["down", "up"])
def test_a_span_near_2_to_the_40(gpu, direction):
    """group g of np outputs reads the stream from g step on: with the material resident there, the span's outputs are the first outputs of
    the material as a stream of its own"""
    _, _, np_, step, hl = DIRECTIONS[direction]
    g = ((1 << 40) - 1) // max(np_, step)                     # the larger of out0 and in0 just below 2^40 (down: out0 is 2^40 147 / 160)
    n_out = 3 * 16 * np_ + 11
    n = (n_out * step) // np_ + 4 * hl
    x = gpu.stream()[:n].contiguous()
    y = gpu.ctx.resample(x, *DIRECTIONS[direction][:2])
    got, used = span(gpu, direction, x, g * step, g * np_, n_out)
    assert used == 1 and max(g * step, g * np_) > (1 << 40) - (1 << 12)
    assert gpu.torch.equal(got, y[:n_out])


@pytest.mark.parametrize("direction", ["down", "up"])
def test_what_takes_k10w_instead(gpu, direction):
    t = gpu.torch
    np_ = DIRECTIONS[direction][2]
    x, y = gpu.stream(), gpu.whole(direction)
    n_out = 16 * np_ + 1
    got, used = span(gpu, direction, x, 0, 1, n_out)                     # not on a multiple of np
    assert used == 0 and t.equal(got, y[1:1 + n_out])
    got, used = span(gpu, direction, x, 0, np_, n_out, shift=1)           # the output 4 bytes off the grid
    assert used == 0 and t.equal(got, y[np_:np_ + n_out])
    off = t.empty((200001,), dtype=t.float32, device="cuda")[1:].view(100000, 2)
    off.copy_(x[:100000])
    got, used = span(gpu, direction, off, 0, np_, n_out)                  # the input 4 bytes off the grid
    assert used == 0 and t.equal(got, y[np_:np_ + n_out])
    mono, ymono = gpu.stream(1, 200000, 6), gpu.whole(direction, 1, 200000, 6)
    got, used = span(gpu, direction, mono, 0, np_, n_out)
    assert used == 0 and t.equal(got, ymono.reshape(-1)[np_:np_ + n_out])
    gpu.awm.lib.awm_debug_set_resample_phase(0)
    try:
        got, used = span(gpu, direction, x, 0, 16 * np_, n_out)           # the switch
    finally:
        gpu.awm.lib.awm_debug_set_resample_phase(1)
    assert used == 0 and t.equal(got, y[16 * np_:16 * np_ + n_out])
