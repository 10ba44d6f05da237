"""add_watermark of ONE input with many payloads at a sample rate other than 44.1 kHz (awm_add_watermark_payloads_d, DESIGN.md section
9.4): the stream goes down to 44.1 kHz once, K2m (delta_only) writes the watermark signals of a pass, K10m takes them up to the rate and
into the outputs (path 2: stereo, 48 kHz, 8-byte aligned pointers) or K10 and K11 do per output (path 1: everything else with fixed-ratio
tables); the loop over the single-payload call remains for the rest (path 0).

Every comparison with the single-payload call is torch.equal: the arithmetic per output is that call's own, value for value, and block
maxima are order-free maxima -- there is no tolerance to choose.  Against the oracle the bars are those of `add` (test_gpu_parity.py).

The shapes are the smallest at which this code can go wrong: K10m's tile is 2560 outputs, a limiter block 48 000 samples, a pass four
outputs.  Inputs are generated on the device; single-payload results are computed once per (input, payload, parameters) and shared."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc
from test_gpu_parity import RMS_TOL

pytestmark = pytest.mark.gpu

PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"
ZEROS = "0" * 32
ONES = "f" * 32
MAX_TOL = 2e-6          # the project's bar for `add` against the oracle beside RMS_TOL (test_gpu_add_payloads.py, test_gpu_placement.py)
R48 = 48000
TILE = 2560             # outputs per tile of K10m
ERR_ARG = -3            # AWM_ERR_ARG (include/awm_hip.h)

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def rms(a, b):
    d = np.asarray(a, np.float64).ravel() - np.asarray(b, np.float64).ravel()
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def payloads(n, seed=5):
    """n distinct 128 bit payloads; payloads (m) is a prefix of payloads (n) for m < n: the single-payload results are shared"""
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
        def make():
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed)
            x = torch.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=torch.float32)
            return ((x * 2 - 1) * amp).contiguous()
        return cached(("noise", seed, n, ch, amp), make)
    g.noise = device_noise
    yield g
    _CACHE.clear()
    awm.set_add_payloads_fused(True)
    awm.set_add_payloads_rate_fused(2)
    awm.set_params()
    orc.set_params()
    ctx.close()


def single(gpu, tag, key, pay, x, rate):
    """what the single-payload call writes; `tag` names the input and the parameters in force"""
    return cached(("single", tag, pay, rate), lambda: gpu.ctx.add_watermark(key, pay, x, sample_rate=rate))


def check(gpu, tag, pays, x, rate, path, key=None):
    """outs[p] == add_watermark (pays[p]) bit for bit, the input is untouched; `path`: what add_payloads_rate_fused_in_use() must report"""
    before = x.clone()
    outs = gpu.ctx.add_watermark_payloads(key, pays, x, sample_rate=rate)
    assert gpu.awm.add_payloads_rate_fused_in_use() == path
    assert gpu.awm.add_payloads_fused_in_use() == 0                   # that query speaks of the 44.1 kHz kernel alone
    assert len(outs) == len(pays)
    for p, pay in enumerate(pays):
        assert outs[p].shape == x.shape
        assert gpu.torch.equal(outs[p], single(gpu, tag, key, pay, x, rate)), f"output {p} of {len(pays)} differs from the single-payload call"
    assert gpu.torch.equal(x, before)
    return outs


# ---- 1. stereo 48 kHz: shared down-resample + K2m + K10m ------------------------------------------------------------------------------
LENGTHS = [1, 17, TILE - 1, TILE, TILE + 1, 5 * TILE + 1, R48 - 1, R48, R48 + 1, 2 * R48 + 5, 12 * R48 + 321]


@pytest.mark.parametrize("amp", [1.0, 0.25], ids=["every_block_ramps", "limiter_skips_everything"])
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(gpu, n, amp):
    """tile and limiter block boundaries; five payloads are passes of 3 + 2, with a payload twice and the two extremes among them"""
    x = gpu.noise(100 + n % 97, n, 2, amp)
    outs = check(gpu, ("len", n, amp), [PAY1, ZEROS, PAY1, ONES, PAY2], x, R48, 2)
    assert gpu.torch.equal(outs[0], outs[2])
    if n > R48:
        assert not gpu.torch.equal(outs[1], outs[3])
    if amp < 1:
        assert max(float(o.abs().max()) for o in outs) < 0.5          # nothing near the ceiling: the limiter's apply pass is the identity


@pytest.mark.parametrize("n", [2 * R48 + 5, 12 * R48 + 321])
@pytest.mark.parametrize("n_pay", [2, 4, 5, 9])
def test_payload_counts(gpu, n_pay, n):
    """one pass of 2, one of 4, 3 + 2, 3 + 3 + 3"""
    outs = check(gpu, ("count", n), payloads(n_pay), gpu.noise(7, n, 2), R48, 2)
    assert not gpu.torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("amp", [1.0, 0.25])
@pytest.mark.parametrize("limiter", [True, False])
def test_limiter_on_and_off(gpu, limiter, amp):
    gpu.awm.set_params(test_no_limiter=not limiter)
    try:
        check(gpu, ("limiter", limiter, amp), payloads(3), gpu.noise(8, 12 * R48 + 321, 2, amp), R48, 2)
    finally:
        gpu.awm.set_params()


# ---- 2. shared down-resample + K2m, then K10 and K11 per output -----------------------------------------------------------------------
@pytest.mark.parametrize("ch,rate", [(1, R48), (3, R48), (2, 32000), (2, 96000), (2, 22050), (2, 88200)])
def test_other_shapes_take_the_separate_kernels(gpu, ch, rate):
    check(gpu, ("shape", ch, rate), payloads(5), gpu.noise(20 + ch, 3 * rate + 77, ch), rate, 1)


GUARD = 4096            # floats on either side of a placed buffer
CANARY = -7.25


@pytest.mark.parametrize("which", ["input", "output 1", "nothing"])
def test_four_byte_alignment_and_guards(gpu, which):
    """stereo 48 kHz with the input or one output 4 bytes off inside a larger tensor: path 1 (path 2 when everything is aligned); every
    output between guard values that stay, the input unchanged"""
    torch = gpu.torch
    n = 3 * R48 + 11
    pays = payloads(3)

    def place(off):
        big = torch.full((GUARD + 2 + 2 * n + GUARD,), CANARY, dtype=torch.float32, device="cuda")
        view = big[GUARD + off:GUARD + off + 2 * n].view(n, 2)
        assert view.is_contiguous() and view.data_ptr() % 8 == 4 * off
        return big, view

    src = gpu.noise(30, n, 2)
    xbig, x = place(1 if which == "input" else 0)
    x.copy_(src)
    bufs = [place(1 if which == "output %d" % p else 0) for p in range(3)]
    gpu.ctx.add_watermark_payloads(None, pays, x, [v for _, v in bufs], sample_rate=R48)
    assert gpu.awm.add_payloads_rate_fused_in_use() == (2 if which == "nothing" else 1)
    for p, (big, view) in enumerate(bufs):
        off = view.storage_offset()
        assert bool((big[:off] == CANARY).all()) and bool((big[off + 2 * n:] == CANARY).all()), f"guards of output {p}"
        assert torch.equal(view, single(gpu, "placed", None, pays[p], src, R48)), f"output {p}"
    off = x.storage_offset()
    assert torch.equal(x, src) and bool((xbig[:off] == CANARY).all()) and bool((xbig[off + 2 * n:] == CANARY).all())


# ---- 3. the loop ----------------------------------------------------------------------------------------------------------------------
def test_one_payload_loops(gpu):
    check(gpu, "loop", payloads(1), gpu.noise(40, 3 * R48 + 5, 2), R48, 0)


def test_vresampler_rate_loops(gpu):
    check(gpu, "loop", payloads(2), gpu.noise(41, 2 * 44101 + 5, 2), 44101, 0)


def test_the_44_1_khz_switch_means_loop_at_every_rate(gpu):
    gpu.awm.set_add_payloads_fused(False)
    try:
        check(gpu, "loop", payloads(3), gpu.noise(40, 3 * R48 + 5, 2), R48, 0)
    finally:
        gpu.awm.set_add_payloads_fused(True)


def test_rate_switch_off_loops(gpu):
    gpu.awm.set_add_payloads_rate_fused(0)
    try:
        check(gpu, "loop", payloads(3), gpu.noise(40, 3 * R48 + 5, 2), R48, 0)
    finally:
        gpu.awm.set_add_payloads_rate_fused(2)


def test_44_1_khz_reports_no_rate_path(gpu):
    gpu.ctx.add_watermark_payloads(None, payloads(2), gpu.noise(42, 44100 + 3, 2))
    assert gpu.awm.add_payloads_fused_in_use() == 1 and gpu.awm.add_payloads_rate_fused_in_use() == 0


# ---- 4. the switch --------------------------------------------------------------------------------------------------------------------
def test_the_three_modes_agree(gpu):
    x = gpu.noise(50, 6 * R48 + 1, 2)
    pays = payloads(5)
    got = {}
    try:
        for mode in (2, 1, 0):
            gpu.awm.set_add_payloads_rate_fused(mode)
            got[mode] = gpu.ctx.add_watermark_payloads(None, pays, x, sample_rate=R48)
            assert gpu.awm.add_payloads_rate_fused_in_use() == mode
    finally:
        gpu.awm.set_add_payloads_rate_fused(2)
    for p in range(len(pays)):
        assert gpu.torch.equal(got[2][p], got[1][p]) and gpu.torch.equal(got[2][p], got[0][p]), f"output {p}"
    assert not gpu.torch.equal(got[2][0], got[2][1])


# ---- 5. the sharing really happens ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pay,want", [(4, (1, 1, 0, 1)), (9, (1, 3, 0, 3))])
def test_launches(gpu, n_pay, want):
    """one down-resample for the call, one K2m and one K10m per pass, no K2 and no further resampler launch"""
    awm, ctx = gpu.awm, gpu.ctx
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    x = gpu.noise(60, 6 * R48, 2)
    pays = payloads(n_pay)
    ctx.synchronize()
    lib.awm_prof_enable(ctx._h, 1)
    try:
        lib.awm_prof_reset(ctx._h)
        ctx.add_watermark_payloads(None, pays, x, sample_rate=R48)
        ctx.synchronize()
        assert awm.add_payloads_rate_fused_in_use() == 2
        counts = {}
        for i in range(lib.awm_prof_count()):
            launches = C.c_long()
            assert lib.awm_prof_read(ctx._h, i, None, C.byref(launches), None) == 0
            counts[lib.awm_prof_name(i).decode()] = launches.value
    finally:
        lib.awm_prof_enable(ctx._h, 0)
    got = (counts["resample_kernel"], counts["add_mix_multi_kernel"], counts["add_mix_kernel"], counts["resample_mix_multi_kernel"])
    assert got == want, counts
    assert counts["limiter_kernel"] == n_pay


# ---- 6. parameters of the context -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [dict(mix=False), dict(frames_per_bit=3)], ids=["linear", "frames_per_bit3"])
def test_parameters_of_the_context(gpu, params):
    gpu.awm.set_params(**params)
    try:
        check(gpu, ("params", str(params)), payloads(3), gpu.noise(70, 8 * R48 + 1, 2), R48, 2)
    finally:
        gpu.awm.set_params()


def test_test_key(gpu):
    check(gpu, "test key", payloads(3), gpu.noise(71, 4 * R48, 2), R48, 2, key=gpu.awm.test_key(42))


# ---- 7. each copy decodes to its own payload; the oracle ------------------------------------------------------------------------------
def test_each_copy_decodes_to_its_own_payload(gpu):
    n = 60 * R48
    x = gpu.noise(80, n, 2)
    pays = [PAY1, PAY2, ONES]
    outs = gpu.ctx.add_watermark_payloads(None, pays, x, sample_rate=R48)
    assert gpu.awm.add_payloads_rate_fused_in_use() == 2
    for p, pay in enumerate(pays):
        bits = [q["bits"] for q in gpu.ctx.get_watermark(None, gpu.ctx.resample(outs[p], R48, 44100))]
        others = [o for o in pays if o != pay]
        print(f"copy {p}: {len(bits)} patterns, {bits.count(pay)} own, {sum(b in others for b in bits)} of another copy")
        assert bits.count(pay) >= 1
        assert not any(b in others for b in bits)


def test_against_oracle(gpu):
    n = 5 * R48 + 3
    x = np.random.default_rng(301).uniform(-1, 1, (n, 2)).astype(np.float32)
    pays = [PAY1, PAY2, ONES]
    outs = gpu.ctx.add_watermark_payloads(None, pays, gpu.dev(x), sample_rate=R48)
    assert gpu.awm.add_payloads_rate_fused_in_use() == 2
    pay = pays[1]
    want = orc.add(None, x, 2, pay, sample_rate=R48).reshape(n, 2)
    got = outs[1].cpu().numpy().reshape(n, 2)
    r, m = rms(got, want), float(np.abs(got - want).max())
    print(f"oracle 48 kHz: rms {r:.3e} max {m:.3e} watermark rms {rms(got, x):.4f}")
    assert r < RMS_TOL
    assert m < MAX_TOL
    assert 0.005 < rms(got, x) < 0.05                          # a watermark was actually embedded


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_alone(gpu):
    torch = gpu.torch
    x = gpu.noise(90, 2 * R48, 2)
    before = x.clone()
    sentinel = 123.5
    outs = [torch.full_like(x, sentinel) for _ in range(3)]

    def untouched():
        gpu.ctx.synchronize()
        return all(bool((o == sentinel).all()) for o in outs)

    def call(pays, x_, outs_):
        hexes = (C.c_char_p * len(pays))(*[p.encode() for p in pays])
        dst = (C.c_void_p * len(pays))(*[o.data_ptr() for o in outs_])
        return gpu.awm.lib.awm_add_watermark_payloads_d(gpu.ctx._h, gpu.awm.key_bytes(None), hexes, len(pays), C.c_void_p(x_.data_ptr()), dst,
                                                        x_.shape[0], 2, R48)

    good = [PAY1, PAY2, ONES]
    assert call(good, x, [outs[0], x, outs[2]]) == ERR_ARG and untouched()             # an output that is the input
    assert call(good, x, [outs[0], outs[1], outs[0]]) == ERR_ARG and untouched()       # two outputs overlap
    assert call([PAY1, "not-hex", PAY2], x, outs) == ERR_ARG and untouched()
    with pytest.raises(gpu.awm.AwmError, match="index 1"):
        gpu.ctx.add_watermark_payloads(None, [PAY1, "not-hex", PAY2], x, outs, sample_rate=R48)
    gpu.ctx.snr_begin()
    try:
        assert call(good, x, outs) == ERR_ARG
    finally:
        gpu.ctx.snr_end()
    assert untouched()
    assert gpu.torch.equal(x, before)
    # and the same call goes through once nothing is wrong with it
    assert call(good, x, outs) == 0
    assert gpu.awm.add_payloads_rate_fused_in_use() == 2 and not untouched()
