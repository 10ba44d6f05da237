"""A batch of stream segments at a sample rate other than 44.1 kHz (awm_add_watermark_segments_rate_d; the reference's HLS mode at the rate of
the programme, hls.cc:279 with WatermarkResampler, wmadd.cc:353-430).

THE DEFINITION every comparison uses, bit for bit (torch.equal): with S = "zero_frames zeros, then the segment", the output is
add_watermark (S, sample_rate)[zero_frames:] -- the whole-stream resampled add, which its own tests pin to the compiled reference.  The
window form runs the same device functions on the same values at the same global indices; there is no tolerance to choose.  Only the
comparisons with the compiled reference itself have bars, the ones tests/test_gpu_streaming.py applies to that comparison (f32: max 4e-6,
RMS 1e-6).

Material is seeded noise x 0.98: the limiter is at work in every block.  Lengths and offsets are the smallest at which this code can go
wrong: segments shorter than a resampler window, a 44.1 kHz frame (1115 samples at 48 kHz) and a limiter block (48000) and their
neighbours, the resampler cycle (160), the table wrap (44.1 kHz frame 249 -> 250 is sample 278 000 at 48 kHz), the second pair of watermark
blocks.  Expected tensors are computed once per (rate, payload, segment, offset) and shared."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R48 = 48000
P48 = 2605056000                     # period of the whole pipeline in zero_frames at 48 kHz: lcm (resampler cycle, table period, limiter block)
WRAP48 = 278000                      # 44.1 kHz frame 249 -> 250: table row 4451 -> 0
SECOND48 = 4969800                   # seven frames into the second pair of watermark blocks
FAR = 3600 * R48 + 12345

LENGTHS = [0, 1, 17, 1023, 1115, R48, R48 + 1, 2 * R48 + 5, 200000]
OFFSETS = [0, 1, 159, 160, 161, 1114, 1115, 3 * 1024 + 17, R48 - 1, R48, R48 + 1, 10 * R48 - 10]
MIXED = ([(LENGTHS[i % 9], OFFSETS[i % 12]) for i in range(20)]
         + [(3000, WRAP48), (200000, WRAP48 - 1500), (R48 + 1, SECOND48), (1023, SECOND48)])

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def payloads(n, seed=21):
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

    def noise(seed, n, ch=2):
        def make():
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed)
            x = torch.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=torch.float32)
            return ((x * 2 - 1) * 0.98).contiguous()
        return cached(("noise", seed, n, ch), make)
    g.noise = noise

    def expected(rate, key, payload, x, seed, zero_frames, tag="default"):
        """the definition: the whole-stream add of "zero_frames zeros, then the segment", cut again"""
        def make():
            if x.shape[0] == 0:
                return x.clone()
            s = torch.zeros((zero_frames + x.shape[0],) + tuple(x.shape[1:]), dtype=torch.float32, device="cuda")
            s[zero_frames:] = x
            w = ctx.add_watermark(key, payload, s, sample_rate=rate)
            ctx.synchronize()
            return w[zero_frames:].clone()
        return cached(("whole", rate, key, payload, seed, tuple(x.shape), zero_frames, tag), make)
    g.expected = expected
    yield g
    _CACHE.clear()
    awm.lib.awm_debug_set_add_batched(2)
    ctx.set_params()
    ctx.close()


def batch(gpu, cases, n_payloads=6, ch=2, seed0=100):
    pays = payloads(n_payloads)
    segs = [gpu.noise(seed0 + i, n, ch) for i, (n, _) in enumerate(cases)]
    return [pays[i % n_payloads] for i in range(len(cases))], segs, [zf for _, zf in cases]


GUARD = 64                           # floats on either side of every output (256 bytes: the outputs stay on the 16-byte grid)


def guarded(gpu, segs, shift=0):
    """an output per segment between guard values; shift: floats the output is moved off the 16-byte grid"""
    t = gpu.torch
    rooms, outs = [], []
    for s in segs:
        room = t.full((2 * GUARD + s.numel() + 4,), float("nan"), dtype=t.float32, device="cuda")
        rooms.append(room)
        outs.append(room[GUARD + shift:GUARD + shift + s.numel()].view(s.shape))
    return rooms, outs


def guards_intact(gpu, rooms, segs, shift=0):
    gpu.ctx.synchronize()
    t = gpu.torch
    return all(bool(t.isnan(r[:GUARD + shift]).all()) and bool(t.isnan(r[GUARD + shift + s.numel():]).all()) for r, s in zip(rooms, segs))


def check(gpu, rate, key, pays, segs, zfs, outs, seed0=100, tag="default"):
    t = gpu.torch
    for i, (p, x, zf, o) in enumerate(zip(pays, segs, zfs, outs)):
        assert o.shape == x.shape
        assert t.equal(o, gpu.expected(rate, key, p, x, seed0 + i, zf, tag)), f"segment {i}: {x.shape[0]} samples at zero_frames {zf}, {rate} Hz"


def fused_mixed(gpu):
    def make():
        pays, segs, zfs = batch(gpu, MIXED)
        before = [s.clone() for s in segs]
        rooms, outs = guarded(gpu, segs)
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=R48)
        gpu.ctx.synchronize()
        fused = gpu.awm.add_segments_fused_in_use()
        assert guards_intact(gpu, rooms, segs), "a guard value next to an output was overwritten"
        assert all(gpu.torch.equal(a, b) for a, b in zip(before, segs)), "an input buffer was written to"
        return outs, fused
    return cached("fused mixed", make)


def test_segments_48k_equal_the_whole_stream_add(gpu):
    pays, segs, zfs = batch(gpu, MIXED)
    assert len(segs) == 24 and len(set(pays)) == 6
    assert set(n for n, _ in MIXED) >= set(LENGTHS) and set(z for _, z in MIXED) >= set(OFFSETS)
    outs, fused = fused_mixed(gpu)
    assert fused == 1
    check(gpu, R48, None, pays, segs, zfs, outs)
    # the offset and the payload both matter
    x = segs[16]
    assert not gpu.torch.equal(outs[16], gpu.expected(R48, None, pays[16 % 6], x, 116, zfs[16] + 1))
    assert not gpu.torch.equal(outs[16], gpu.expected(R48, None, pays[0], x, 116, zfs[16]))


def test_misaligned_pointers_fall_back(gpu):
    """the same batch with every pointer four bytes off the 16-byte grid: segment by segment through the single-stream launchers"""
    t = gpu.torch
    pays, segs, zfs = batch(gpu, MIXED)
    shifted = []
    for s in segs:
        room = t.empty(s.numel() + 1, dtype=t.float32, device="cuda")
        v = room[1:].view(s.shape)
        v.copy_(s)
        assert s.numel() == 0 or v.data_ptr() % 16 == 4
        shifted.append(v)
    rooms, outs = guarded(gpu, segs, shift=1)
    assert all(o.data_ptr() % 16 == 4 for o in outs if o.numel())
    gpu.ctx.add_watermark_segments(None, pays, shifted, zfs, outs, sample_rate=R48)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    assert guards_intact(gpu, rooms, segs, shift=1)
    check(gpu, R48, None, pays, segs, zfs, outs)


@pytest.mark.parametrize("rate", [32000, 96000])
def test_rates_whose_first_stage_goes_up(gpu, rate):
    """32 kHz (hl 23 on the way down to it) and 96 kHz (hl 35 on the way down from it): the generic windowed kernel in both directions"""
    frame = 1024 * rate // 44100
    cases = [(17, 1), (1023, frame + 1), (rate + 1, rate - 1), (2 * rate + 5, 3 * 1024 + 17), (40000, 10 * rate - 10),
             (3 * frame + 100, 250 * 1024 * rate // 44100 - frame)]
    pays, segs, zfs = batch(gpu, cases, n_payloads=3, seed0=200 + rate // 1000)
    rooms, outs = guarded(gpu, segs)
    gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=rate)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    assert guards_intact(gpu, rooms, segs)
    check(gpu, rate, None, pays, segs, zfs, outs, seed0=200 + rate // 1000)


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "single"])
def test_loud_material_raises_the_block_maxima_in_front_of_the_segment(gpu, fused):
    """In the whole-stream add the watermark begins ~2 frames in front of the segment (the frame that holds its first sample shapes the one
    before it, and the resamplers ring).  With samples of +-300 that stretch alone exceeds the limiter's ceiling, so the maxima of the block
    of zero_frames AND of the block before it (zero_frames just behind a block edge) change the ramps inside the segment: the window form
    has to compute that stretch, it cannot start at zero_frames"""
    cases = [(5000, R48 + 50), (3 * R48, 7 * R48 + 1200), (1115, 3), (R48, 5 * R48 - 20)]
    pays, segs, zfs = batch(gpu, cases, n_payloads=2, seed0=450)
    loud = [cached(("loud", i), lambda s=s: (s * 300).contiguous()) for i, s in enumerate(segs)]
    plan = gpu.awm.add_segment_plan(R48, zfs[0], 5000)
    assert plan["mix_first"] < R48 and plan["first_block"] == 0              # (the stretch reaches back into the block before)
    if fused:
        outs = gpu.ctx.add_watermark_segments(None, pays, loud, zfs, sample_rate=R48)
    else:
        outs = [gpu.ctx.add_watermark_segments(None, [p], [x], [z], sample_rate=R48)[0] for p, x, z in zip(pays, loud, zfs)]
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == fused
    check(gpu, R48, None, pays, loud, zfs, outs, seed0=450, tag="loud")
    # the stretch is what matters here: an add of the segment's block alone, without it, scales the first samples differently
    s = gpu.torch.zeros((50 + 5000, 2), device="cuda")
    s[50:] = loud[0]
    alone = gpu.ctx.add_watermark(None, pays[0], s, sample_rate=R48)[50:]
    assert not gpu.torch.equal(alone[:1000], outs[0][:1000])


@pytest.mark.parametrize("ch", [1, 3])
def test_other_channel_counts_fall_back(gpu, ch):
    cases = [(17, 159), (1115, 1114), (R48 + 1, R48 - 1), (2 * R48 + 5, 3 * 1024 + 17), (0, 5)]
    pays, segs, zfs = batch(gpu, cases, n_payloads=2, ch=ch, seed0=400 + ch)
    rooms, outs = guarded(gpu, segs)
    gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=R48)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    assert guards_intact(gpu, rooms, segs)
    check(gpu, R48, None, pays, segs, zfs, outs, seed0=400 + ch)


def test_the_toggle_and_a_single_segment_fall_back(gpu):
    pays, segs, zfs = batch(gpu, MIXED)
    pick = [4, 7, 11, 20]
    p, s, z = [pays[i] for i in pick], [segs[i] for i in pick], [zfs[i] for i in pick]
    gpu.awm.lib.awm_debug_set_add_batched(0)
    try:
        outs = gpu.ctx.add_watermark_segments(None, p, s, z, sample_rate=R48)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 0
    finally:
        gpu.awm.lib.awm_debug_set_add_batched(2)
    for j, i in enumerate(pick):
        assert gpu.torch.equal(outs[j], gpu.expected(R48, None, p[j], s[j], 100 + i, z[j]))
    one = gpu.ctx.add_watermark_segments(None, p[1:2], s[1:2], z[1:2], sample_rate=R48)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    assert gpu.torch.equal(one[0], outs[1])


# ---- aliasing inputs and the launch structure -----------------------------------------------------------------------------------------
def scopes(gpu, call):
    """{scope: (launches, algorithmic bytes)} of one call"""
    lib, ctx = gpu.awm.lib, gpu.ctx
    lib.awm_prof_name.restype = C.c_char_p
    ctx.synchronize()
    lib.awm_prof_enable(ctx._h, 1)
    try:
        lib.awm_prof_reset(ctx._h)
        result = call()
        ctx.synchronize()
        out = {}
        for i in range(lib.awm_prof_count()):
            launches, nbytes = C.c_long(), C.c_double()
            assert lib.awm_prof_read(ctx._h, i, None, C.byref(launches), C.byref(nbytes)) == 0
            out[lib.awm_prof_name(i).decode()] = (launches.value, nbytes.value)
    finally:
        lib.awm_prof_enable(ctx._h, 0)
    return result, out


def test_one_segment_for_five_subscribers_shares_its_slice(gpu):
    pays = payloads(5, seed=22)
    n, zf = 2 * R48 + 5, 3 * 1024 + 17
    x = gpu.noise(300, n)
    before = x.clone()
    outs, sc = scopes(gpu, lambda: gpu.ctx.add_watermark_segments(None, pays, [x] * 5, [zf] * 5, sample_rate=R48))
    assert gpu.awm.add_segments_fused_in_use() == 1
    for p, o in zip(pays, outs):
        single = gpu.ctx.add_watermark_segments(None, [p], [x], [zf], sample_rate=R48)[0]
        gpu.ctx.synchronize()
        assert gpu.torch.equal(o, single)
        assert gpu.torch.equal(o, gpu.expected(R48, None, p, x, 300, zf))
    assert gpu.torch.equal(before, x) and not gpu.torch.equal(outs[0], outs[1])
    # the resample scope: two launches (down, up); the down-resampler read the segment and wrote its 44.1 kHz slice ONCE, the up-resampler
    # read five watermark signals and wrote five
    plan = gpu.awm.add_segment_plan(R48, zf, n)
    down = (plan["in_last"] - plan["in_first"] + 1) + (plan["slice_last"] - plan["slice_first"] + 1) * 1024
    up = (plan["frame_last"] - plan["frame_first"] + 1) * 1024 + (zf - plan["mix_first"]) + n
    assert sc["resample_kernel"] == (2, (down + 5 * up) * 2 * 4.0)


def launch_counts(gpu, n_segments):
    cases = [(5000 + 37 * i, [0, 1115, WRAP48, R48 - 1, 7 * 1024][i % 5]) for i in range(n_segments)]
    pays, segs, zfs = batch(gpu, cases, n_payloads=n_segments, seed0=500)
    outs, sc = scopes(gpu, lambda: gpu.ctx.add_watermark_segments(None, pays, segs, zfs, sample_rate=R48))
    assert gpu.awm.add_segments_fused_in_use() == 1
    check(gpu, R48, None, pays[:3], segs[:3], zfs[:3], outs[:3], seed0=500)
    return {k: v[0] for k, v in sc.items()}


def test_launches_do_not_depend_on_the_number_of_segments(gpu):
    few, many = launch_counts(gpu, 3), launch_counts(gpu, 40)
    assert few["payload_table_kernel"] == many["payload_table_kernel"] == 1
    assert few["resample_kernel"] == many["resample_kernel"] == 2
    assert few["add_mix_kernel"] == many["add_mix_kernel"] == 1
    assert few["limiter_kernel"] == many["limiter_kernel"] == 1
    assert few == many


# ---- parameter sets of the context ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [dict(frames_per_bit=3), dict(mix=False), dict(test_no_limiter=1)], ids=["frames_per_bit3", "linear", "no_limiter"])
def test_segments_with_parameters_of_the_context(gpu, params):
    cases = [(1115, 1114), (2 * R48 + 5, WRAP48 - 1500), (40000, 10 * R48 - 10), (1023, R48)]
    tag = tuple(params.items())
    gpu.ctx.set_params(**params)
    try:
        pays, segs, zfs = batch(gpu, cases, n_payloads=3, seed0=340)
        outs = gpu.ctx.add_watermark_segments(None, pays, segs, zfs, sample_rate=R48)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 1
        check(gpu, R48, None, pays, segs, zfs, outs, seed0=340, tag=tag)
    finally:
        gpu.ctx.set_params()
    assert not gpu.torch.equal(outs[1], gpu.expected(R48, None, pays[1], segs[1], 341, zfs[1]))
    if "test_no_limiter" in params:
        assert float(outs[1].abs().max()) > 1.0


# ---- the splits of a call ---------------------------------------------------------------------------------------------------------------
def check_split_call(gpu, n, n_payloads, seed, parts, sample):
    """one call that has to be split equals the same segments in calls that are not, and the segments of `sample` equal the definition"""
    t = gpu.torch
    pool = gpu.noise(seed, 8192)
    pays = payloads(n_payloads, seed=seed)
    pays = [pays[i % n_payloads] for i in range(n)]
    segs = [pool[2 * (i * 7 % 2000):][:64] for i in range(n)]
    zfs = [(i * 5 % 300) * 1115 + i * 11 % 1115 for i in range(n)]
    whole = gpu.ctx.add_watermark_segments(None, pays, segs, zfs, sample_rate=R48)
    assert gpu.awm.add_segments_fused_in_use() == 1
    pieces = []
    for a, b in parts:
        assert b - a <= 4096 and len(set(pays[a:b])) <= 1024
        pieces += gpu.ctx.add_watermark_segments(None, pays[a:b], segs[a:b], zfs[a:b], sample_rate=R48)
    gpu.ctx.synchronize()
    bad = [i for i in range(n) if not t.equal(whole[i], pieces[i])]
    assert not bad, f"segments {bad[:8]} differ between the split call and the unsplit ones"
    for i in sample:
        assert t.equal(whole[i], gpu.expected(R48, None, pays[i], segs[i], (seed, i), zfs[i])), f"segment {i} at zero_frames {zfs[i]}"


def test_more_segments_than_a_launch(gpu):
    check_split_call(gpu, 4097, 6, 701, [(0, 2048), (2048, 4097)], [0, 3, 4095, 4096])


def test_more_payloads_than_a_table_group(gpu):
    check_split_call(gpu, 1025, 1025, 700, [(0, 512), (512, 1025)], [0, 1023, 1024])


def test_more_watermark_frames_than_a_workspace(gpu):
    """twelve subscribers of one 300 s segment: one shared 44.1 kHz slice, but twelve watermark signals of 27 M floats each -- more than
    the 2^28 floats of a workspace, so the batch is split; every output equals the single call"""
    t = gpu.torch
    n, zf = 300 * R48, 5 * R48 + 77
    x = gpu.noise(900, n)
    pays = payloads(12, seed=23)
    assert 12 * ((n * 147 // 160) // 1024) * 1024 * 2 > 2 ** 28
    outs = gpu.ctx.add_watermark_segments(None, pays, [x] * 12, [zf] * 12, sample_rate=R48)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    single = t.empty_like(x)
    for p, o in zip(pays, outs):
        gpu.ctx.add_watermark_segments(None, [p], [x], [zf], [single], sample_rate=R48)
        gpu.ctx.synchronize()
        assert t.equal(o, single)
    assert t.equal(outs[11], gpu.expected(R48, None, pays[11], x, 900, zf))


# ---- far offsets: the zeros cannot be materialised --------------------------------------------------------------------------------------
def test_the_pipeline_is_periodic_in_zero_frames(gpu):
    """Z and Z + P give the same output bit for bit (the compiled reference has exactly this period): every index product crosses 2^31
    and 2^32 on the way"""
    pays = payloads(2, seed=24)
    x, y = gpu.noise(800, 2 * R48 + 5), gpu.noise(801, 1115)
    Z = 144100
    outs = gpu.ctx.add_watermark_segments(None, pays * 2, [x, y, x, y], [Z, Z + 7, Z + P48, Z + 7 + P48], sample_rate=R48)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    assert gpu.torch.equal(outs[0], outs[2]) and gpu.torch.equal(outs[1], outs[3])
    assert gpu.torch.equal(outs[0], gpu.expected(R48, None, pays[0], x, 800, Z))
    assert gpu.torch.equal(outs[1], gpu.expected(R48, None, pays[1], y, 801, Z + 7))
    one = gpu.ctx.add_watermark_segments(None, pays[:1], [x], [Z + P48], sample_rate=R48)      # ... and through the single-stream launchers
    gpu.ctx.synchronize()
    assert gpu.torch.equal(one[0], outs[0])


@pytest.mark.parametrize("zf", [FAR, 0, R48 - 1, 10 * R48 - 10], ids=["one_hour", "start", "block_edge", "ten_seconds"])
def test_against_the_compiled_reference(gpu, zf):
    """the reference's own add_stream_watermark (..., zero_frames) at 48 kHz, under the bars of tests/test_gpu_streaming.py for float
    output: max 4e-6, RMS 1e-6"""
    import _ref
    if not _ref.available():
        pytest.skip("oracle/_ref is not built")
    pays = payloads(2, seed=25)
    x, y = gpu.noise(810, 2 * R48 + 5), gpu.noise(811, 1115)
    outs = gpu.ctx.add_watermark_segments(None, pays, [x, y], [zf, zf], sample_rate=R48)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    ref = _ref.add_at(None, x.cpu().numpy(), 2, pays[0], zf, sample_rate=R48).reshape(-1, 2)
    assert ref.shape == tuple(x.shape)
    d = outs[0].cpu().numpy().astype(np.float64) - ref
    print("zero_frames %d: rms %.3g max %.3g" % (zf, np.sqrt((d ** 2).mean()), np.abs(d).max()))
    assert np.abs(d).max() <= 4e-6 and np.sqrt((d ** 2).mean()) < 1e-6


# ---- refusals: AWM_ERR_ARG, nothing enqueued ---------------------------------------------------------------------------------------------
def refusal_batch(gpu):
    t = gpu.torch
    pays, segs, zfs = batch(gpu, [(3 * 1024 + 17, 1023), (5000, 1115), (1025, R48 - 1)], n_payloads=3, seed0=600)
    outs = [t.full_like(s, float("nan")) for s in segs]
    return pays, segs, zfs, outs


def untouched(gpu, outs):
    gpu.ctx.synchronize()
    return all(bool(gpu.torch.isnan(o).all()) for o in outs)


@pytest.mark.parametrize("rate,what", [(44101, "fixed-ratio"), (0, "sample rate"), (-48000, "sample rate")])
def test_refuses_a_rate_without_a_table(gpu, rate, what):
    pays, segs, zfs, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match=what):
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=rate)
    assert untouched(gpu, outs)


def test_refuses_an_offset_beyond_2_to_the_40(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match="segment 1.*2\\^40"):
        gpu.ctx.add_watermark_segments(None, pays, segs, [zfs[0], 2 ** 40 - 5000, zfs[2]], outs, sample_rate=R48)
    assert untouched(gpu, outs)
    gpu.ctx.add_watermark_segments(None, pays, segs, [zfs[0], 2 ** 40 - 5001, zfs[2]], outs, sample_rate=R48)       # the largest offset taken
    gpu.ctx.synchronize()
    assert not untouched(gpu, outs) and bool(gpu.torch.isfinite(outs[1]).all())


def test_refuses_an_output_that_overlaps_an_input(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match="overlaps"):
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, [outs[0], segs[1], outs[2]], sample_rate=R48)          # in place
    with pytest.raises(gpu.awm.AwmError, match="overlaps"):
        gpu.ctx.add_watermark_segments(None, pays[:2], [segs[1], segs[1]], zfs[:2], [outs[1], outs[1]], sample_rate=R48)
    assert untouched(gpu, outs)


def test_refuses_a_payload_that_does_not_parse(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match="index 2"):
        gpu.ctx.add_watermark_segments(None, [pays[0], pays[1], "xyz"], segs, zfs, outs, sample_rate=R48)
    assert untouched(gpu, outs)


def test_refuses_a_call_while_the_snr_meter_is_armed(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    gpu.ctx.snr_begin()
    try:
        with pytest.raises(gpu.awm.AwmError, match="SNR"):
            gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=R48)
    finally:
        gpu.ctx.snr_end()
    assert untouched(gpu, outs)
    gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=R48)
    check(gpu, R48, None, pays, segs, zfs, outs, seed0=600)


def test_no_segments_and_the_watermark_rate(gpu):
    lib = gpu.awm.lib
    assert lib.awm_add_watermark_segments_rate_d(gpu.ctx._h, bytes(16), 0, None, None, None, None, None, 2, R48) == 0
    pays, segs, zfs, _ = refusal_batch(gpu)
    a = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
    n = len(segs)
    outs = [gpu.torch.empty_like(s) for s in segs]
    rc = lib.awm_add_watermark_segments_rate_d(gpu.ctx._h, bytes(16), n, (C.c_char_p * n)(*[p.encode() for p in pays]), (C.c_size_t * n)(*zfs),
                                               (C.c_void_p * n)(*[s.data_ptr() for s in segs]), (C.c_void_p * n)(*[o.data_ptr() for o in outs]),
                                               (C.c_size_t * n)(*[s.shape[0] for s in segs]), 2, 44100)
    gpu.ctx.synchronize()
    assert rc == 0 and all(gpu.torch.equal(x, y) for x, y in zip(a, outs))


# ---- the file level: a stream that continues an hour in -----------------------------------------------------------------------------------
def file_add(gpu, tmp_path, x, zero_frames, name):
    """awm_add_stream_watermark_file of float32 raw PCM on a context of its own -> (output, device bytes the call allocated)"""
    awm, t = gpu.awm, gpu.torch
    ctx = awm.Context(0)
    try:
        raw_in = ctx.pcm_encode(x.reshape(-1), 32, 2, False, True).cpu().numpy()
        src, dst = tmp_path / (name + "_in.raw"), tmp_path / (name + "_out.raw")
        raw_in.tofile(src)
        rf = awm.binding.RawFormat(2, R48, 32, 2, 0)
        ctx.synchronize()
        before = awm.lib.awm_debug_alloc_bytes()
        ctx.add_watermark_file(None, payloads(1, seed=26)[0], src, dst, rf, rf, zero_frames=zero_frames)
        allocated = awm.lib.awm_debug_alloc_bytes() - before
        got = ctx.pcm_decode(t.from_numpy(np.fromfile(dst, np.uint8)).cuda(), 32, 2, False).reshape(-1, 2).clone()
    finally:
        ctx.close()
    return got, allocated


def test_file_add_an_hour_into_a_stream(gpu, tmp_path):
    import _ref
    x = gpu.noise(820, 2 * R48)
    far, far_bytes = file_add(gpu, tmp_path, x, FAR, "far")
    near, near_bytes = file_add(gpu, tmp_path, x, 100, "near")
    assert far.shape == near.shape == tuple(x.shape)
    print("device bytes allocated: zero_frames %d: %d, zero_frames 100: %d" % (FAR, far_bytes, near_bytes))
    assert far_bytes == near_bytes and far_bytes < 1 << 30            # (an hour of zeros alone would be 1.4 GB)
    pay = payloads(1, seed=26)[0]
    assert gpu.torch.equal(far, gpu.ctx.add_watermark_segments(None, [pay], [x], [FAR], sample_rate=R48)[0])
    assert gpu.torch.equal(near, gpu.expected(R48, None, pay, x, 820, 100))
    if not _ref.available():
        pytest.skip("oracle/_ref is not built")
    ref = _ref.add_at(None, x.cpu().numpy(), 2, pay, FAR, sample_rate=R48).reshape(-1, 2)
    d = far.cpu().numpy().astype(np.float64) - ref
    assert np.abs(d).max() <= 4e-6 and np.sqrt((d ** 2).mean()) < 1e-6


def test_file_add_with_a_meter_the_caller_armed(gpu, tmp_path):
    """awm_ctx_snr_begin: "every add of this context accumulates ... until snr_end".  The window form refuses a call while the meter is
    armed, so the file level keeps the whole-stream path then: the call succeeds as it always did, writes the same bytes, and the meter
    reports the powers of the whole-stream add of "zero_frames zeros, then the file" (sums of doubles in any order: 1e-9 relative)"""
    awm, t = gpu.awm, gpu.torch
    zf, pay = 144100, payloads(1, seed=26)[0]
    x = gpu.noise(830, 2 * R48)
    plain, _ = file_add(gpu, tmp_path, x, zf, "plain")
    ctx = awm.Context(0)
    try:
        raw_in = ctx.pcm_encode(x.reshape(-1), 32, 2, False, True).cpu().numpy()
        src, dst = tmp_path / "armed_in.raw", tmp_path / "armed_out.raw"
        raw_in.tofile(src)
        rf = awm.binding.RawFormat(2, R48, 32, 2, 0)
        ctx.snr_begin()
        ctx.add_watermark_file(None, pay, src, dst, rf, rf, zero_frames=zf)
        snr_file = ctx.snr_end()
        armed = ctx.pcm_decode(t.from_numpy(np.fromfile(dst, np.uint8)).cuda(), 32, 2, False).reshape(-1, 2).clone()
        s = t.zeros((zf + x.shape[0], 2), device="cuda")
        s[zf:] = x
        ctx.snr_begin()
        ctx.add_watermark(None, pay, s, sample_rate=R48)
        snr_whole = ctx.snr_end()
    finally:
        ctx.close()
    assert t.equal(armed, plain)
    assert np.isfinite(snr_file) and snr_file == pytest.approx(snr_whole, rel=1e-9)
