"""add_watermark of ONE input with many payloads (awm_add_watermark_payloads_d, kernel K2m): every output is bit for bit what
awm_add_watermark_d writes for that payload -- the fused kernel runs the same device functions and expressions as K2, so there is
no tolerance anywhere in the comparisons with the single-payload path.  Against the oracle the bars are those of `add`
(test_gpu_parity.py); each copy must decode to its own payload and to none of its neighbours'.

Large inputs are generated on the device (seeded torch generator), so that no case waits for the CPU or for PCIe."""
import numpy as np
import pytest

import _oracle as orc

pytestmark = pytest.mark.gpu

PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"
ZEROS = "0" * 32
ONES = "f" * 32
RMS_TOL = 1e-6          # the project's bars for `add` against the oracle (test_gpu_parity.py)
MAX_TOL = 2e-6
SR = 44100


def rms(a, b):
    d = np.asarray(a, np.float64).ravel() - np.asarray(b, np.float64).ravel()
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def payloads(n, seed=5):
    """n distinct 128 bit payloads"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = rng.integers(0, 256, 16, dtype=np.uint8).tobytes().hex()
        if p not in out:
            out.append(p)
    return out


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

    def device_noise(seed, n, ch, amp=1.0):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        x = torch.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=torch.float32)
        return ((x * 2 - 1) * amp).contiguous()
    g.noise = device_noise
    yield g
    awm.set_add_payloads_fused(True)
    awm.set_params()
    orc.set_params()
    ctx.close()


def check_equals_single(gpu, key, pays, x, fused, sample_rate=SR):
    """outs[p] == add_watermark (pays[p]) bit for bit; `fused`: the value add_payloads_fused_in_use() must report"""
    outs = gpu.ctx.add_watermark_payloads(key, pays, x, sample_rate=sample_rate)
    assert gpu.awm.add_payloads_fused_in_use() == fused
    assert len(outs) == len(pays)
    for p, pay in enumerate(pays):
        want = gpu.ctx.add_watermark(key, pay, x, sample_rate=sample_rate)
        assert outs[p].shape == x.shape
        assert gpu.torch.equal(outs[p], want), f"output {p} of {len(pays)} differs from the single-payload path"
        del want
    return outs


# ---- 1. bit-identical to the single-payload path ------------------------------------------------------------------------------
@pytest.mark.parametrize("ch,n,n_pay", [
    (2, 70 * SR + 13, 2),               # stereo, a tail that is no whole frame
    (1, 20 * SR + 1, 3),                # mono: the one-channel body
    (3, 4 * SR + 5, 3),                 # three channels: a channel per wave
    (2, 1, 3), (2, 700, 3), (2, 1024, 3), (2, 1025, 3), (1, 1025, 2)])
def test_equals_single_payload(gpu, ch, n, n_pay):
    x = gpu.noise(200 + ch + n % 89, n, ch)
    check_equals_single(gpu, None, payloads(n_pay), x, fused=1)


def test_more_than_two_tile_passes(gpu):
    """3 PT + 1 payloads: four passes over the input, not a multiple of the tile"""
    pt = gpu.awm.ADD_PAYLOADS_TILE
    assert pt >= 1
    x = gpu.noise(11, 30 * SR, 2)
    check_equals_single(gpu, None, payloads(3 * pt + 1), x, fused=1)


def test_one_payload_is_the_single_path(gpu):
    x = gpu.noise(12, 10 * SR + 3, 2)
    outs = gpu.ctx.add_watermark_payloads(None, [PAY1], x)
    assert len(outs) == 1 and gpu.torch.equal(outs[0], gpu.ctx.add_watermark(None, PAY1, x))


@pytest.mark.parametrize("limiter", [True, False])
@pytest.mark.parametrize("ch", [2, 1])
def test_limiter_on_and_off(gpu, limiter, ch):
    gpu.awm.set_params(test_no_limiter=not limiter)
    try:
        check_equals_single(gpu, None, payloads(3), gpu.noise(13 + ch, 12 * SR + 7, ch), fused=1)
    finally:
        gpu.awm.set_params()


def test_test_key(gpu):
    check_equals_single(gpu, gpu.awm.test_key(42), payloads(3), gpu.noise(14, 12 * SR, 2), fused=1)


@pytest.mark.parametrize("params", [dict(mix=False), dict(frames_per_bit=3)], ids=["linear", "frames_per_bit3"])
def test_parameters_of_the_context(gpu, params):
    gpu.awm.set_params(**params)
    try:
        check_equals_single(gpu, None, payloads(3), gpu.noise(15, 25 * SR + 1, 2), fused=1)
    finally:
        gpu.awm.set_params()


def test_same_payload_twice_and_extremes(gpu):
    x = gpu.noise(16, 20 * SR, 2)
    outs = check_equals_single(gpu, None, [PAY1, ZEROS, PAY1, ONES, ZEROS], x, fused=1)
    assert gpu.torch.equal(outs[0], outs[2]) and gpu.torch.equal(outs[1], outs[4])
    assert not gpu.torch.equal(outs[1], outs[3])


@pytest.mark.parametrize("amp", [1.0, 0.25], ids=["every_block_ramps", "limiter_skips_everything"])
def test_amplitudes(gpu, amp):
    x = gpu.noise(17, 30 * SR + 100, 2, amp)
    outs = check_equals_single(gpu, None, payloads(3), x, fused=1)
    if amp < 1:
        assert max(float(o.abs().max()) for o in outs) < 0.5               # nothing near the ceiling: the limiter's apply pass is the identity


def test_other_sample_rate_loops(gpu):
    """48 kHz: the resampled add is not fused (a loop over the single-payload path), the results are the same"""
    check_equals_single(gpu, None, payloads(2), gpu.noise(18, 10 * 48000, 2), fused=0, sample_rate=48000)


def test_sixty_minutes_stereo(gpu):
    """60 min: long spans (about 50 frames instead of the minimum of 4), every CU full, two tile passes (3 + 2 outputs)"""
    x = gpu.noise(19, 60 * 60 * SR, 2)
    outs = check_equals_single(gpu, None, payloads(5), x, fused=1)
    assert not gpu.torch.equal(outs[0], outs[1])


# ---- 2. against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch,n", [(2, 30 * SR), (1, 20 * SR)])
def test_against_oracle(gpu, ch, n):
    x = np.random.default_rng(300 + ch).uniform(-1, 1, (n, ch)).astype(np.float32)
    pays = [PAY1, PAY2, ONES]
    outs = gpu.ctx.add_watermark_payloads(None, pays, gpu.dev(x))
    assert gpu.awm.add_payloads_fused_in_use() == 1
    for p, pay in enumerate(pays):
        want = orc.add(None, x, ch, pay).reshape(n, ch)
        got = outs[p].cpu().numpy().reshape(n, ch)
        r, m = rms(got, want), float(np.abs(got - want).max())
        print(f"oracle ch={ch} payload {p}: rms {r:.3e} max {m:.3e} watermark rms {rms(got, x):.4f}")
        assert r < RMS_TOL
        assert m < MAX_TOL
        assert 0.005 < rms(got, x) < 0.05                      # a watermark was actually embedded


# ---- 3. each copy decodes to its own payload ----------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", [1.0, 0.25])
def test_each_copy_decodes_to_its_own_payload(gpu, amp):
    n = 120 * SR
    x = (np.random.default_rng(3).uniform(-1, 1, (n, 2)) * amp).astype(np.float32)
    pays = [PAY1, PAY2, ZEROS, ONES]
    outs = gpu.ctx.add_watermark_payloads(None, pays, gpu.dev(x))
    assert gpu.awm.add_payloads_fused_in_use() == 1
    for p, pay in enumerate(pays):
        bits = [q["bits"] for q in gpu.ctx.get_watermark(None, outs[p])]
        others = [o for o in pays if o != pay]
        print(f"amp {amp} copy {p}: {len(bits)} patterns, {bits.count(pay)} own, {sum(b in others for b in bits)} of another copy")
        assert bits.count(pay) >= 1
        assert not any(b in others for b in bits)


# ---- 4. the fallback loop equals the fused kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [2, 1])
def test_fallback_equals_fused(gpu, ch):
    x = gpu.noise(20 + ch, 15 * SR + 9, ch)
    pays = payloads(5)
    fused = gpu.ctx.add_watermark_payloads(None, pays, x)
    assert gpu.awm.add_payloads_fused_in_use() == 1
    gpu.awm.set_add_payloads_fused(False)
    try:
        loop = gpu.ctx.add_watermark_payloads(None, pays, x)
        assert gpu.awm.add_payloads_fused_in_use() == 0
    finally:
        gpu.awm.set_add_payloads_fused(True)
    for a, b in zip(fused, loop):
        assert gpu.torch.equal(a, b)


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_alone(gpu):
    torch = gpu.torch
    x = gpu.noise(21, 3 * SR, 2)
    sentinel = 123.5
    outs = [torch.full_like(x, sentinel) for _ in range(3)]

    def untouched():
        gpu.ctx.synchronize()
        return all(bool((o == sentinel).all()) for o in outs)

    with pytest.raises(gpu.awm.AwmError, match="index 1"):                  # bad hex in position 2 of 3
        gpu.ctx.add_watermark_payloads(None, [PAY1, "not-hex", PAY2], x, outs)
    assert untouched()
    with pytest.raises(gpu.awm.AwmError, match="output 1 overlaps the input"):
        gpu.ctx.add_watermark_payloads(None, [PAY1, PAY2, ONES], x, [outs[0], x, outs[2]])
    assert untouched()
    with pytest.raises(gpu.awm.AwmError, match="outputs 0 and 2 overlap"):
        gpu.ctx.add_watermark_payloads(None, [PAY1, PAY2, ONES], x, [outs[0], outs[1], outs[0]])
    assert untouched()
    gpu.ctx.snr_begin()
    try:
        with pytest.raises(gpu.awm.AwmError, match="SNR"):
            gpu.ctx.add_watermark_payloads(None, [PAY1, PAY2, ONES], x, outs)
    finally:
        gpu.ctx.snr_end()
    assert untouched()
    # and the same call goes through once nothing is wrong with it
    gpu.ctx.add_watermark_payloads(None, [PAY1, PAY2, ONES], x, outs)
    assert not untouched()


def test_empty_calls(gpu):
    torch = gpu.torch
    x = gpu.noise(22, SR, 2)
    assert gpu.ctx.add_watermark_payloads(None, [], x) == []
    e = torch.zeros((0, 2), dtype=torch.float32, device="cuda")
    outs = gpu.ctx.add_watermark_payloads(None, [PAY1, PAY2], e)
    assert [tuple(o.shape) for o in outs] == [(0, 2), (0, 2)]
    with pytest.raises(ValueError):
        gpu.ctx.add_watermark_payloads(None, [PAY1, PAY2], x, [torch.empty_like(x)])
    with pytest.raises(ValueError):
        gpu.ctx.add_watermark_payloads(None, [PAY1], x, [torch.empty_like(x, dtype=torch.float64)])
