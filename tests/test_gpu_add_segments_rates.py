"""Segment batches with a sample rate per segment (awm_add_watermark_segments_rates_d and its keys / 16-bit twins).

THE DEFINITION every comparison uses, bit for bit (torch.equal): out[i] is what the one-rate call of the same family writes for segment i
ALONE at sample_rates[i] -- and those calls are pinned to the whole-stream add and to the compiled reference by
tests/test_gpu_add_segments_rate.py, test_gpu_add_segments.py, test_gpu_add_segments_keys.py and test_gpu_add_segments_s16.py.  There is no
tolerance anywhere in this file.

Material is seeded noise x 0.98: the limiter is at work in every block.  Per rate R the lengths and offsets are the smallest at which the
code can go wrong: the cycle U of the resampler on the way up (np of the table 44100 -> R), a 44.1 kHz frame (F = ceil (1024 R / 44100)
samples), the limiter block (R samples) and their neighbours, the table wrap inside a segment.  Outputs sit between NaN guards (16-bit:
sentinel values), inputs must come back unchanged.  Expected tensors are computed once per (rate, key, payload, segment, offset)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATES = [48000, 32000, 96000, 22050, 88200, 44100]
OTHER = RATES[:5]
GUARD = 64                           # values on either side of every output (the outputs stay on the 16-byte grid)
SENTINEL = 23130                     # 0x5a5a

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def payloads(n, seed=31):
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

    def noise(seed, n, ch=2, level=0.98):
        def make():
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed)
            x = torch.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=torch.float32)
            return ((x * 2 - 1) * level).contiguous()
        return cached(("noise", seed, n, ch, level), make)
    g.noise = noise

    def single(rate, key, payload, x, seed, zero_frames, tag="default"):
        """the definition: the one-rate call for the segment alone"""
        def make():
            out = ctx.add_watermark_segments(key, [payload], [x], [zero_frames], sample_rate=rate)[0]
            ctx.synchronize()
            assert awm.add_segments_fused_in_use() == 0
            return out
        return cached(("single", rate, key, payload, seed, tuple(x.shape), zero_frames, tag), make)
    g.single = single
    yield g
    _CACHE.clear()
    awm.lib.awm_debug_set_add_batched(2)
    ctx.set_params()
    ctx.close()


def geometry(gpu, rate):
    """(U, F) of a rate; at 44.1 kHz a frame and the cycle of the 48 kHz table"""
    if rate == 44100:
        return 160, 1024
    return gpu.awm.add_segment_plan(rate, 0, 0)["up_np"], -(-1024 * rate // 44100)


def lengths_of(gpu, rate):
    _, F = geometry(gpu, rate)
    return [0, 1, 17, 1023, F, rate - 1, rate, rate + 1, 2 * rate + 5]


def offsets_of(gpu, rate):
    U, F = geometry(gpu, rate)
    return [0, 1, U - 1, U, U + 1, F - 1, F, 3 * 1024 + 17, rate - 1, rate, rate + 1, 10 * rate - 10, -(-256000 * rate // 44100) - 1500]


def mixed_cases(gpu, n=36):
    """(rate, length, offset, length index, offset index) per segment: the rates cycle, every rate meets six lengths and six offsets"""
    cases = []
    for i in range(n):
        r, j = i % 6, i // 6
        rate = RATES[r]
        li, oi = (j + 2 * r) % 9, (2 * j + 5 * r) % 13
        if oi == 12:
            li = 8                                         # the table wrap lies INSIDE the segment: 2 R + 5 samples from 1500 in front of it
        cases.append((rate, lengths_of(gpu, rate)[li], offsets_of(gpu, rate)[oi], li, oi))
    return cases


def batch(gpu, cases, n_payloads=6, ch=2, seed0=100, level=0.98):
    pays = payloads(n_payloads)
    segs = [gpu.noise(seed0 + i, c[1], ch, level) for i, c in enumerate(cases)]
    return [pays[i % n_payloads] for i in range(len(cases))], segs, [c[2] for c in cases], [c[0] for c in cases]


def guarded(gpu, segs, shift=0):
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


def check(gpu, keys, pays, segs, zfs, rates, outs, seed0=100, tag="default"):
    t = gpu.torch
    for i, (p, x, zf, rate, o) in enumerate(zip(pays, segs, zfs, rates, outs)):
        key = keys[i] if isinstance(keys, list) else keys
        assert o.shape == x.shape
        assert t.equal(o, gpu.single(rate, key, p, x, seed0 + i, zf, tag)), f"segment {i}: {x.shape[0]} samples at zero_frames {zf}, {rate} Hz"


def run_guarded(gpu, pays, segs, zfs, rates, keys=None, per_key=False):
    before = [s.clone() for s in segs]
    rooms, outs = guarded(gpu, segs)
    if per_key:
        gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs, outs, sample_rate=rates)
    else:
        gpu.ctx.add_watermark_segments(keys, pays, segs, zfs, outs, sample_rate=rates)
    gpu.ctx.synchronize()
    fused = gpu.awm.add_segments_fused_in_use()
    assert guards_intact(gpu, rooms, segs), "a guard value next to an output was overwritten"
    assert all(gpu.torch.equal(a, b) for a, b in zip(before, segs)), "an input buffer was written to"
    return outs, fused


def fused_mixed(gpu):
    def make():
        pays, segs, zfs, rates = batch(gpu, mixed_cases(gpu))
        return run_guarded(gpu, pays, segs, zfs, rates)
    return cached("fused mixed", make)


# ---- 1, 2: the mixed batch ---------------------------------------------------------------------------------------------------------------
def test_the_mixed_batch_equals_the_one_rate_single_calls(gpu):
    cases = mixed_cases(gpu)
    pays, segs, zfs, rates = batch(gpu, cases)
    assert len(segs) == 36 and len(set(pays)) == 6 and set(rates) == set(RATES)
    assert {c[3] for c in cases} == set(range(9)) and {c[4] for c in cases} == set(range(13))
    for rate in RATES:
        mine = [c for c in cases if c[0] == rate]
        assert len(mine) == 6 and len({c[4] for c in mine}) == 6 and len({c[3] for c in mine}) >= 5
    outs, fused = fused_mixed(gpu)
    assert fused == 1
    check(gpu, None, pays, segs, zfs, rates, outs)
    # the rate matters: the same samples at the same offset at another rate are another stream
    i = next(k for k, c in enumerate(cases) if c[0] == 48000 and c[1] >= 40000)
    assert not gpu.torch.equal(outs[i], gpu.single(32000, None, pays[i], segs[i], 100 + i, zfs[i]))


def test_the_reversed_batch_gives_the_reversed_outputs(gpu):
    pays, segs, zfs, rates = batch(gpu, mixed_cases(gpu))
    outs, _ = fused_mixed(gpu)
    back, fused = run_guarded(gpu, pays[::-1], segs[::-1], zfs[::-1], rates[::-1])
    assert fused == 1
    for i, (a, b) in enumerate(zip(outs, back[::-1])):
        assert gpu.torch.equal(a, b), f"segment {i}"


# ---- 3: the fallbacks, same bits ----------------------------------------------------------------------------------------------------------
def test_misaligned_pointers_fall_back(gpu):
    t = gpu.torch
    pays, segs, zfs, rates = batch(gpu, mixed_cases(gpu))
    shifted = []
    for s in segs:
        room = t.empty(s.numel() + 1, dtype=t.float32, device="cuda")
        v = room[1:].view(s.shape)
        v.copy_(s)
        assert s.numel() == 0 or v.data_ptr() % 16 == 4
        shifted.append(v)
    rooms, outs = guarded(gpu, segs, shift=1)
    gpu.ctx.add_watermark_segments(None, pays, shifted, zfs, outs, sample_rate=rates)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    assert guards_intact(gpu, rooms, segs, shift=1)
    check(gpu, None, pays, segs, zfs, rates, outs)


@pytest.mark.parametrize("ch", [1, 3])
def test_other_channel_counts_fall_back(gpu, ch):
    cases = mixed_cases(gpu, 12)
    pays, segs, zfs, rates = batch(gpu, cases, n_payloads=3, ch=ch, seed0=400 + 20 * ch)
    rooms, outs = guarded(gpu, segs)
    gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=rates)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    assert guards_intact(gpu, rooms, segs)
    check(gpu, None, pays, segs, zfs, rates, outs, seed0=400 + 20 * ch)


def test_the_toggle_falls_back(gpu):
    pays, segs, zfs, rates = batch(gpu, mixed_cases(gpu))
    pick = [6, 7, 13, 20, 27, 35]
    p, s, z, r = [pays[i] for i in pick], [segs[i] for i in pick], [zfs[i] for i in pick], [rates[i] for i in pick]
    gpu.awm.lib.awm_debug_set_add_batched(0)
    try:
        outs = gpu.ctx.add_watermark_segments(None, p, s, z, sample_rate=r)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 0
    finally:
        gpu.awm.lib.awm_debug_set_add_batched(2)
    for j, i in enumerate(pick):
        assert gpu.torch.equal(outs[j], gpu.single(r[j], None, p[j], s[j], 100 + i, z[j]))


def test_a_rate_below_the_batched_limiters_bound_falls_back(gpu):
    assert gpu.awm.add_segment_plan(8000, 0, 0)["limiter_block"] == 8000
    cases = [(48000, 5000, 1115), (8000, 8000 + 17, 8000 - 1), (32000, 1023, 32000), (44100, 3000, 1025)]
    pays, segs, zfs, rates = batch(gpu, cases, n_payloads=2, seed0=480)
    outs, fused = run_guarded(gpu, pays, segs, zfs, rates)
    assert fused == 0
    check(gpu, None, pays, segs, zfs, rates, outs, seed0=480)
    outs, fused = run_guarded(gpu, pays[:1] + pays[2:], segs[:1] + segs[2:], zfs[:1] + zfs[2:], rates[:1] + rates[2:])
    assert fused == 1                                       # (the 8 kHz segment alone kept the batch off the fused path)


def test_slices_whose_window_does_not_fit_take_the_unstaged_taps_in_the_same_launch(gpu):
    """176.4 and 192 kHz on the way down: a tile of 1024 outputs reads more than 4096 input frames, so K10w does not stage the window for
    these slices (the table stays in LDS) -- per slice, beside the staged 48 and 32 kHz slices of the same launch"""
    for rate in (176400, 192000):
        plan = gpu.awm.add_segment_plan(rate, 0, 0)
        assert 1023 * plan["down_step"] // plan["down_np"] + 2 + 2 * plan["down_hl"] > 4096
    plan = gpu.awm.add_segment_plan(48000, 0, 0)
    assert 1023 * plan["down_step"] // plan["down_np"] + 2 + 2 * plan["down_hl"] <= 4096
    cases = [(176400, 176400 + 1, 176400 - 1), (48000, 5000, 1115), (192000, 3 * 4459 + 100, 4459 + 1), (32000, 32000 + 1, 743),
             (176400, 1023, 3 * 1024 + 17), (192000, 192000 + 1, 10 * 192000 - 10), (44100, 3000, 1025)]
    pays, segs, zfs, rates = batch(gpu, cases, n_payloads=3, seed0=900)
    outs, fused = run_guarded(gpu, pays, segs, zfs, rates)
    assert fused == 1
    check(gpu, None, pays, segs, zfs, rates, outs, seed0=900)


# ---- 4, 5: what is shared, and the launch structure ---------------------------------------------------------------------------------------
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


def test_one_input_at_two_rates_makes_two_down_slices(gpu):
    pays = payloads(6, seed=32)
    n, zf = 2 * 32000 + 5, 3 * 1024 + 17
    x = gpu.noise(300, n)
    before = x.clone()
    rates = [48000, 32000, 48000, 32000, 48000, 32000]
    outs, sc = scopes(gpu, lambda: gpu.ctx.add_watermark_segments(None, pays, [x] * 6, [zf] * 6, sample_rate=rates))
    assert gpu.awm.add_segments_fused_in_use() == 1
    for p, rate, o in zip(pays, rates, outs):
        assert gpu.torch.equal(o, gpu.single(rate, None, p, x, 300, zf))
    assert gpu.torch.equal(before, x) and not gpu.torch.equal(outs[0], outs[2])
    # the resample scope: two launches (down, up); the down-resampler read the input and wrote a 44.1 kHz slice ONCE PER RATE, the
    # up-resampler read six watermark signals and wrote six
    total = 0
    for rate in (48000, 32000):
        plan = gpu.awm.add_segment_plan(rate, zf, n)
        down = (plan["in_last"] - plan["in_first"] + 1) + (plan["slice_last"] - plan["slice_first"] + 1) * 1024
        up = (plan["frame_last"] - plan["frame_first"] + 1) * 1024 + (zf - plan["mix_first"]) + n
        total += down + 3 * up
    assert sc["resample_kernel"] == (2, total * 2 * 4.0)


def launch_counts(gpu, n_segments, rates_of):
    cases = []
    for i in range(n_segments):
        rate = rates_of[i % len(rates_of)]
        _, F = geometry(gpu, rate)
        cases.append((rate, 5000 + 37 * i, [0, F, rate - 1, 7 * 1024, 250 * F][i // len(rates_of) % 5]))
    pays, segs, zfs, rates = batch(gpu, cases, n_payloads=n_segments, seed0=500)
    if len(set(rates)) == 1:
        rates = rates[0]
    outs, sc = scopes(gpu, lambda: gpu.ctx.add_watermark_segments(None, pays, segs, zfs, sample_rate=rates))
    assert gpu.awm.add_segments_fused_in_use() == 1
    return {k: v[0] for k, v in sc.items()}


def test_launches_do_not_depend_on_the_number_of_segments_or_of_rates(gpu):
    few, many = launch_counts(gpu, 6, OTHER), launch_counts(gpu, 60, OTHER)
    assert few["payload_table_kernel"] == many["payload_table_kernel"] == 1
    assert few["resample_kernel"] == many["resample_kernel"] == 2
    assert few["add_mix_kernel"] == many["add_mix_kernel"] == 1
    assert few["limiter_kernel"] == many["limiter_kernel"] == 1
    assert few == many
    assert launch_counts(gpu, 60, [48000]) == many
    few44, many44 = launch_counts(gpu, 6, RATES), launch_counts(gpu, 60, RATES)
    assert few44["payload_table_kernel"] == many44["payload_table_kernel"] == 1
    assert few44 == many44 and few44["add_mix_kernel"] == 2


# ---- 6: a key per segment -------------------------------------------------------------------------------------------------------------
def test_keys_at_several_rates_build_their_templates_once(gpu):
    awm = gpu.awm
    three = [None, awm.test_key(7), bytes(range(16))]
    four = [48000, 32000, 44100, 88200]
    cases, keys = [], []
    for i in range(12):
        rate = four[(i + i // 4) % 4]                       # key i % 3 meets all four rates
        _, F = geometry(gpu, rate)
        cases.append((rate, [1023, rate + 1, 5000, 3 * F + 100][i % 4], [F + 1, rate - 1, 3 * 1024 + 17, 10 * rate - 10][i // 3 % 4]))
        keys.append(three[i % 3])
    for k in range(3):
        assert len({c[0] for i, c in enumerate(cases) if i % 3 == k}) >= 2
    pays, segs, zfs, rates = batch(gpu, cases, n_payloads=5, seed0=620)
    (outs, fused), sc = scopes(gpu, lambda: run_guarded(gpu, pays, segs, zfs, rates, keys, per_key=True))
    assert fused == 1
    check(gpu, keys, pays, segs, zfs, rates, outs, seed0=620)
    assert sc["key_template_kernel"][0] == 1 and sc["payload_table_kernel"][0] == 1
    same, fused = run_guarded(gpu, pays, segs, zfs, rates, [three[1]] * 12, per_key=True)
    assert fused == 1
    one, fused = run_guarded(gpu, pays, segs, zfs, rates, three[1])
    assert fused == 1
    for a, b in zip(same, one):
        assert gpu.torch.equal(a, b)
    check(gpu, three[1], pays, segs, zfs, rates, one, seed0=620)


# ---- 7: 16-bit PCM ------------------------------------------------------------------------------------------------------------------------
def s16_cases(gpu):
    cases = []
    for i in range(12):
        rate = RATES[i % 6]
        _, F = geometry(gpu, rate)
        cases.append((rate, [1023, rate + 1, 3 * F + 101, 5000][i % 4], [F + 1, rate - 1, 3 * 1024 + 17][i % 3]))
    return cases


def pcm16(gpu, seed, n):
    return cached(("pcm16", seed, n), lambda: gpu.torch.round(gpu.noise(seed, n) * 32767).to(gpu.torch.int16).contiguous())


def rooms16(gpu, segs, shift=None):
    """an int16 output per segment between sentinels; shift[i]: values the output is moved off the 16-byte grid"""
    t = gpu.torch
    shift = shift or [0] * len(segs)
    rooms, outs = [], []
    for s, sh in zip(segs, shift):
        room = t.full((2 * GUARD + s.numel() + 8,), SENTINEL, dtype=t.int16, device="cuda")
        rooms.append(room)
        outs.append(room[GUARD + sh:GUARD + sh + s.numel()].view(s.shape))
    return rooms, outs


def sentinels_intact(gpu, rooms, segs, shift=None):
    gpu.ctx.synchronize()
    shift = shift or [0] * len(segs)
    return all(bool((r[:GUARD + sh] == SENTINEL).all()) and bool((r[GUARD + sh + s.numel():] == SENTINEL).all())
               for r, s, sh in zip(rooms, segs, shift))


def run16(gpu, keys, pays, ins, zfs, rates, per_key, shift=None):
    before = [s.clone() for s in ins]
    rooms, outs = rooms16(gpu, ins, shift)
    if per_key:
        gpu.ctx.add_watermark_segments_keys_s16(keys, pays, ins, zfs, outs, sample_rate=rates)
    else:
        gpu.ctx.add_watermark_segments_s16(keys, pays, ins, zfs, outs, sample_rate=rates)
    gpu.ctx.synchronize()
    fused = gpu.awm.add_segments_fused_in_use()
    assert sentinels_intact(gpu, rooms, ins, shift), "a value outside an output's n C values was written"
    assert all(gpu.torch.equal(a, b) for a, b in zip(before, ins)), "an input buffer was written to"
    return outs, fused


@pytest.mark.parametrize("per_key", [False, True], ids=["one_key", "keys"])
def test_16_bit_segments_equal_the_definition_and_the_single_calls(gpu, per_key):
    t, ctx, awm = gpu.torch, gpu.ctx, gpu.awm
    cases = s16_cases(gpu)
    pays = [payloads(4, seed=33)[i % 4] for i in range(12)]
    ins = [pcm16(gpu, 700 + i, c[1]) for i, c in enumerate(cases)]
    zfs, rates = [c[2] for c in cases], [c[0] for c in cases]
    keys = [[None, awm.test_key(9)][i % 2] for i in range(12)] if per_key else awm.test_key(9)
    outs, fused = run16(gpu, keys, pays, ins, zfs, rates, per_key)
    assert fused == 1
    # the definition: decode, the float mixed call, encode (direct16)
    fs = [ctx.pcm_decode(x.view(t.uint8).reshape(-1), 16).reshape(x.shape) for x in ins]
    if per_key:
        gs = ctx.add_watermark_segments_keys(keys, pays, fs, zfs, sample_rate=rates)
    else:
        gs = ctx.add_watermark_segments(keys, pays, fs, zfs, sample_rate=rates)
    assert awm.add_segments_fused_in_use() == 1
    for i, (g, o) in enumerate(zip(gs, outs)):
        want = ctx.pcm_encode(g.reshape(-1), 16, direct16=True).view(t.int16).reshape(o.shape)
        assert t.equal(o, want), f"segment {i} against the definition"
    # the one-rate 16-bit call for every segment alone
    for i, o in enumerate(outs):
        key = keys[i] if per_key else keys
        alone = ctx.add_watermark_segments_s16(key, [pays[i]], [ins[i]], [zfs[i]], sample_rate=rates[i])[0]
        ctx.synchronize()
        assert t.equal(o, alone), f"segment {i} against the one-rate call"
    # one pointer that is only 2-byte aligned: segment by segment, the same values
    shift = [0] * 12
    shift[5] = 1
    back, fused = run16(gpu, keys, pays, ins, zfs, rates, per_key, shift)
    assert fused == 0 and back[5].data_ptr() % 4 == 2
    for a, b in zip(outs, back):
        assert t.equal(a, b)


def test_16_bit_segments_without_rates_are_at_44100(gpu):
    cases = s16_cases(gpu)[:4]
    pays = payloads(4, seed=33)
    ins = [pcm16(gpu, 700 + i, c[1]) for i, c in enumerate(cases)]
    zfs = [c[2] for c in cases]
    none, fused = run16(gpu, None, pays, ins, zfs, None, False)
    assert fused == 1
    want = gpu.ctx.add_watermark_segments_s16(None, pays, ins, zfs, sample_rate=44100)
    gpu.ctx.synchronize()
    for a, b in zip(none, want):
        assert gpu.torch.equal(a, b)
    keys = [None, gpu.awm.test_key(9), None, gpu.awm.test_key(9)]
    none, _ = run16(gpu, keys, pays, ins, zfs, None, True)
    want = gpu.ctx.add_watermark_segments_keys_s16(keys, pays, ins, zfs, sample_rate=44100)
    gpu.ctx.synchronize()
    for a, b in zip(none, want):
        assert gpu.torch.equal(a, b)


# ---- 8: loud material ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "fallback"])
def test_loud_material_raises_the_block_maxima_in_front_of_each_segment(gpu, fused):
    """samples of +-300: the stretch mix_first .. Z - 1 of watermark alone exceeds the ceiling, so the maxima of the block of zero_frames and
    of the one before it change the ramps inside the segment -- with each segment's OWN block size (48000 and 32000 samples in one batch)"""
    cases = [(48000, 5000, 48000 + 50), (32000, 5000, 32000 + 50), (48000, 3 * 48000, 7 * 48000 + 1200), (32000, 3 * 32000, 7 * 32000 + 800),
             (32000, 743, 3), (48000, 48000, 5 * 48000 - 20), (32000, 32000, 5 * 32000 - 20)]
    pays, segs, zfs, rates = batch(gpu, cases, n_payloads=2, seed0=450, level=0.98 * 300)
    for rate, n, zf in cases[:2]:
        plan = gpu.awm.add_segment_plan(rate, zf, n)
        assert plan["mix_first"] < rate and plan["first_block"] == 0          # (the stretch reaches back into the block before)
    gpu.awm.lib.awm_debug_set_add_batched(2 if fused else 0)
    try:
        outs, used = run_guarded(gpu, pays, segs, zfs, rates)
    finally:
        gpu.awm.lib.awm_debug_set_add_batched(2)
    assert used == fused
    check(gpu, None, pays, segs, zfs, rates, outs, seed0=450, tag="loud")
    # the block size is the segment's own: the 32 kHz segment's samples at 48 kHz scale differently
    assert not gpu.torch.equal(outs[1], gpu.single(48000, None, pays[1], segs[1], 451, zfs[1], "loud"))


# ---- 9: parameter sets of the context -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [dict(frames_per_bit=3), dict(mix=False), dict(test_no_limiter=1)], ids=["frames_per_bit3", "linear", "no_limiter"])
def test_segments_with_parameters_of_the_context(gpu, params):
    cases = mixed_cases(gpu, 12)
    tag = tuple(params.items())
    gpu.ctx.set_params(**params)
    try:
        pays, segs, zfs, rates = batch(gpu, cases, n_payloads=3, seed0=340)
        outs, fused = run_guarded(gpu, pays, segs, zfs, rates)
        assert fused == 1
        check(gpu, None, pays, segs, zfs, rates, outs, seed0=340, tag=tag)
    finally:
        gpu.ctx.set_params()
    i = next(k for k, c in enumerate(cases) if c[1] >= 22050)
    assert not gpu.torch.equal(outs[i], gpu.single(rates[i], None, pays[i], segs[i], 340 + i, zfs[i]))


# ---- 10: the splits of a call -----------------------------------------------------------------------------------------------------------
def check_split_call(gpu, n, n_payloads, seed, some_rates):
    """one mixed call that has to be split equals one one-rate call per rate over the sorted segments"""
    t = gpu.torch
    pool = gpu.noise(seed, 8192)
    pays = payloads(n_payloads, seed=seed)
    pays = [pays[i % n_payloads] for i in range(n)]
    segs = [pool[2 * (i * 7 % 2000):][:17] for i in range(n)]
    rates = [some_rates[i % len(some_rates)] for i in range(n)]
    zfs = [(i * 5 % 300) * 1115 + i * 11 % 1115 for i in range(n)]
    whole = gpu.ctx.add_watermark_segments(None, pays, segs, zfs, sample_rate=rates)
    assert gpu.awm.add_segments_fused_in_use() == 1
    for rate in some_rates:
        idx = [i for i in range(n) if rates[i] == rate]
        part = gpu.ctx.add_watermark_segments(None, [pays[i] for i in idx], [segs[i] for i in idx], [zfs[i] for i in idx], sample_rate=rate)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 1
        bad = [i for i, o in zip(idx, part) if not t.equal(whole[i], o)]
        assert not bad, f"segments {bad[:8]} at {rate} Hz differ between the mixed call and the one-rate call"


def test_more_segments_than_a_launch(gpu):
    check_split_call(gpu, 4097, 6, 701, [48000, 32000])


def test_more_payloads_than_a_table_group(gpu):
    check_split_call(gpu, 1025, 1025, 700, [48000, 44100, 96000])


# ---- 11: forwarding -------------------------------------------------------------------------------------------------------------------
def test_equal_rates_are_the_one_rate_call(gpu):
    lib = gpu.awm.lib
    cases = [(48000, 5000, 1115), (48000, 48001, 47999), (48000, 1023, 3 * 1024 + 17)]
    pays, segs, zfs, rates = batch(gpu, cases, n_payloads=3, seed0=800)
    a, sa = scopes(gpu, lambda: gpu.ctx.add_watermark_segments(None, pays, segs, zfs, sample_rate=rates))
    b, sb = scopes(gpu, lambda: gpu.ctx.add_watermark_segments(None, pays, segs, zfs, sample_rate=48000))
    assert sa == sb and all(gpu.torch.equal(x, y) for x, y in zip(a, b))
    a, sa = scopes(gpu, lambda: gpu.ctx.add_watermark_segments(None, pays, segs, zfs, sample_rate=[44100] * 3))
    b, sb = scopes(gpu, lambda: gpu.ctx.add_watermark_segments(None, pays, segs, zfs))
    assert sa == sb and all(gpu.torch.equal(x, y) for x, y in zip(a, b))
    for name in ("awm_add_watermark_segments_rates_d", "awm_add_watermark_segments_keys_rates_d", "awm_add_watermark_segments_rates_s16_d",
                 "awm_add_watermark_segments_keys_rates_s16_d"):
        assert getattr(lib, name)(gpu.ctx._h, bytes(16), 0, None, None, None, None, None, 2, None) == 0


# ---- 12: refusals: AWM_ERR_ARG, nothing enqueued --------------------------------------------------------------------------------------
def refusal_batch(gpu):
    t = gpu.torch
    cases = [(48000, 3 * 1024 + 17, 1023), (32000, 5000, 1115), (44100, 1025, 47999), (96000, 2000, 96000), (48000, 0, 7)]
    pays, segs, zfs, rates = batch(gpu, cases, n_payloads=3, seed0=600)
    outs = [t.full_like(s, float("nan")) for s in segs]
    return pays, segs, zfs, rates, outs


def untouched(gpu, outs):
    gpu.ctx.synchronize()
    return all(bool(gpu.torch.isnan(o).all()) for o in outs)


ARG = "rc=-3.*"                      # AWM_ERR_ARG, as binding._check reports it


def test_refuses_rates_that_are_null(gpu):
    pays, segs, zfs, rates, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match=ARG + "sample_rates is null"):
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=None)
    with pytest.raises(gpu.awm.AwmError, match=ARG + "sample_rates is null"):
        gpu.ctx.add_watermark_segments_keys([None, gpu.awm.test_key(7)] * 2 + [None], pays, segs, zfs, outs, sample_rate=None)
    assert untouched(gpu, outs)


@pytest.mark.parametrize("rate,what", [(44101, "fixed-ratio"), (0, "sample rate"), (-1, "sample rate")])
def test_refuses_a_rate_without_a_table(gpu, rate, what):
    pays, segs, zfs, rates, outs = refusal_batch(gpu)
    bad = rates[:3] + [rate] + rates[4:]
    with pytest.raises(gpu.awm.AwmError, match=ARG + what + ".*index 3"):
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=bad)
    bad = rates[:4] + [rate]                                # (the rate of an empty segment is still checked)
    with pytest.raises(gpu.awm.AwmError, match=ARG + what + ".*index 4"):
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=bad)
    assert untouched(gpu, outs)


def test_refuses_an_offset_beyond_2_to_the_40(gpu):
    pays, segs, zfs, rates, outs = refusal_batch(gpu)
    assert rates[1] == 32000
    far = zfs[:1] + [2 ** 40 - 5000] + zfs[2:]
    with pytest.raises(gpu.awm.AwmError, match=ARG + "segment 1.*2\\^40"):
        gpu.ctx.add_watermark_segments(None, pays, segs, far, outs, sample_rate=rates)
    rates2 = [48000, 44100, 32000, 96000, 48000]
    far = zfs[:2] + [2 ** 40 - 1025] + zfs[3:]
    with pytest.raises(gpu.awm.AwmError, match=ARG + "segment 2.*2\\^40"):
        gpu.ctx.add_watermark_segments(None, pays, segs, far, outs, sample_rate=rates2)
    assert untouched(gpu, outs)
    far = zfs[:2] + [2 ** 40 - 1026] + zfs[3:]                                   # the largest offset taken
    gpu.ctx.add_watermark_segments(None, pays, segs, far, outs, sample_rate=rates2)
    gpu.ctx.synchronize()
    assert not untouched(gpu, outs) and bool(gpu.torch.isfinite(outs[2]).all())


def test_refuses_an_output_that_overlaps_an_input_of_another_rate(gpu):
    pays, segs, zfs, rates, outs = refusal_batch(gpu)
    assert rates[0] != rates[1]
    with pytest.raises(gpu.awm.AwmError, match=ARG + "overlaps"):
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, [segs[1][:segs[0].shape[0]], outs[1], outs[2], outs[3], outs[4]], sample_rate=rates)
    with pytest.raises(gpu.awm.AwmError, match=ARG + "overlaps"):
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, [outs[0], segs[1], outs[2], outs[3], outs[4]], sample_rate=rates)   # in place
    assert untouched(gpu, outs)


def test_refuses_a_payload_that_does_not_parse(gpu):
    pays, segs, zfs, rates, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match=ARG + "index 2"):
        gpu.ctx.add_watermark_segments(None, pays[:2] + ["xyz"] + pays[3:], segs, zfs, outs, sample_rate=rates)
    assert untouched(gpu, outs)


def test_refuses_a_call_while_the_snr_meter_is_armed(gpu):
    pays, segs, zfs, rates, outs = refusal_batch(gpu)
    gpu.ctx.snr_begin()
    try:
        with pytest.raises(gpu.awm.AwmError, match=ARG + "SNR"):
            gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=rates)
    finally:
        gpu.ctx.snr_end()
    assert untouched(gpu, outs)
    gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs, sample_rate=rates)
    check(gpu, None, pays, segs, zfs, rates, outs, seed0=600)


def test_refuses_keys_that_are_null(gpu):
    lib = gpu.awm.lib
    pays, segs, zfs, rates, outs = refusal_batch(gpu)
    n = len(segs)
    args = ((C.c_char_p * n)(*[p.encode() for p in pays]), (C.c_size_t * n)(*zfs), (C.c_void_p * n)(*[s.data_ptr() for s in segs]),
            (C.c_void_p * n)(*[o.data_ptr() for o in outs]), (C.c_size_t * n)(*[s.shape[0] for s in segs]), 2, (C.c_int * n)(*rates))
    for name in ("awm_add_watermark_segments_rates_d", "awm_add_watermark_segments_keys_rates_d"):
        rc = getattr(lib, name)(gpu.ctx._h, None, n, *args)
        assert rc == -3 and rc == lib.awm_add_watermark_segments_rate_d(gpu.ctx._h, None, n, *args[:-1], 48000)
        assert b"bad argument" in lib.awm_last_error()
    assert untouched(gpu, outs)
