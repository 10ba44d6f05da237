"""Segment batches from and to signed 16-bit PCM: awm_add_watermark_segments_rate_s16_d and awm_add_watermark_segments_keys_rate_s16_d
(include/awm_hip.h).

THE DEFINITION every comparison uses, with integer equality (np.array_equal on int16): f_i = pcm_decode (segment i), g_i = what the float
call -- add_watermark_segments, or add_watermark_segments_keys -- writes for the inputs f_i, expected_i = pcm_encode (g_i, 16, direct16),
all three on the same context.  There is no tolerance to choose.

Material is seeded uniform noise rounded to int16 at three levels: amplitude 0.17 (-20 dBFS RMS), full scale (the mix exceeds the limiter's
ceiling in every block) and the quiet one with a stretch of digital silence.  Segments are 13 000 - 110 000 frames: one or two limiter
block edges.  Every call's inputs and outputs sit in a guarded arena (tests/_placement.py); the canaries are checked after every call.

THE RAILS.  The limiter's ceiling is 0.99 and its ramp never lets a value of a block exceed ceiling / block maximum x block maximum, so a
LIMITED value encodes to at most 0.99 x 32768 = 32440: with the limiter on, the saturation of the encode cannot be reached.  The loud
case therefore runs twice -- with the limiter (the definition's output must show the ramp: it differs from the un-limited one and stays
inside +-32440 while the un-limited mix leaves +-1) and with test_no_limiter (the definition's output must hold both 32767 and -32768)."""
import ctypes as C

import numpy as np
import pytest

from _placement import Arena, need

pytestmark = pytest.mark.gpu

R44, R48 = 44100, 48000
HOUR48 = 3600 * R48
QUIET, LOUD = 0.17, 1.0

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
    yield g
    _CACHE.clear()
    awm.lib.awm_debug_set_add_batched(2)
    ctx.set_params()
    ctx.close()


def pcm16(gpu, seed, n, ch=2, level=QUIET, silence=None):
    """host int16 [n, ch] (mono: [n]): the existing noise generator at `level`, rounded; silence = (first, count) frames of zeros"""
    def make():
        t = gpu.torch
        gen = t.Generator(device="cuda")
        gen.manual_seed(seed)
        x = t.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=t.float32)
        v = t.round((x * 2 - 1) * level * 32767).to(t.int16)
        if silence:
            v[silence[0]:silence[0] + silence[1]] = 0
        return v.cpu().numpy()
    return cached(("pcm16", seed, n, ch, level, silence), make)


def definition(gpu, rate, keys, pays, host, zfs, per_key=False):
    """decode, the float call, encode (direct16) on the same context -> list of host int16 arrays"""
    t, ctx = gpu.torch, gpu.ctx
    fs = []
    for h in host:
        raw = t.from_numpy(np.ascontiguousarray(h)).cuda().view(t.uint8).reshape(-1)
        fs.append(ctx.pcm_decode(raw, 16).reshape(h.shape))
    if per_key:
        gs = ctx.add_watermark_segments_keys(keys, pays, fs, zfs, sample_rate=rate)
    else:
        gs = ctx.add_watermark_segments(keys, pays, fs, zfs, sample_rate=rate)
    out = []
    for g, h in zip(gs, host):
        enc = ctx.pcm_encode(g.reshape(-1), 16, direct16=True)
        out.append(enc.cpu().numpy().view(np.int16).reshape(h.shape))
    ctx.synchronize()
    return out, [g.cpu().numpy() for g in gs]


def placed(gpu, host, in_off=None, out_off=None):
    """the call's buffers in one guarded arena: an input per DISTINCT host array (the same array twice is one buffer: aliasing inputs),
    an output per segment; byte offsets from the 256-byte grid per segment (default 0)"""
    t = gpu.torch
    n = len(host)
    in_off, out_off = in_off or [0] * n, out_off or [0] * n
    distinct = {}
    for h in host:
        distinct.setdefault(id(h), h)
    arena = Arena(t, need(*([h.nbytes for h in distinct.values()] + [h.nbytes for h in host])), device="cuda")
    ins_by_id = {}
    for h, o in zip(host, in_off):
        if id(h) not in ins_by_id:
            ins_by_id[id(h)] = arena.place(h, t.int16, o)
    ins = [ins_by_id[id(h)] for h in host]
    outs = [arena.place(h.shape, t.int16, o) for h, o in zip(host, out_off)]
    return arena, ins, outs


def run(gpu, rate, keys, pays, host, zfs, per_key=False, in_off=None, out_off=None):
    """the 16-bit call on guarded buffers -> (host outputs, fused in use); canaries intact, inputs unchanged"""
    arena, ins, outs = placed(gpu, host, in_off, out_off)
    if per_key:
        gpu.ctx.add_watermark_segments_keys_s16(keys, pays, ins, zfs, outs, sample_rate=rate)
    else:
        gpu.ctx.add_watermark_segments_s16(keys, pays, ins, zfs, outs, sample_rate=rate)
    gpu.ctx.synchronize()
    fused = gpu.awm.add_segments_fused_in_use()
    arena.check()
    for x, h in zip(ins, host):
        assert np.array_equal(x.cpu().numpy(), h), "an input buffer was written to"
    return [o.cpu().numpy() for o in outs], fused


def assert_equal(got, want, note=""):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int16 and a.shape == b.shape
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
            raise AssertionError(f"{note} segment {i}: {bad.size} of {a.size} values differ, first at value {bad[0]}: "
                                 f"{a.reshape(-1)[bad[0]]} != {b.reshape(-1)[bad[0]]}")


# ---- 1, 2: the two fused paths ------------------------------------------------------------------------------------------------------------
def batch_44(gpu):
    lengths = [13001, 20000, 30001, 44100 + 777, 110000, 13000, 52001, 20000]
    zfs = [0, 1024 * 3, 1024 * 5 + 1, 1024 * 7 + 1023, 44100 * 2 - 1, 1024 * 40 + 513, 44100 * 3 - 1, 1024 * 9]
    host = [pcm16(gpu, 100 + i, n, silence=(4000, 6000) if i == 2 else None) for i, n in enumerate(lengths)]
    host[7] = host[1]                                       # two segments alias one input
    pays = payloads(3)
    return [pays[i % 3] for i in range(8)], host, zfs


def test_segments_at_44100_equal_the_definition(gpu):
    pays, host, zfs = batch_44(gpu)
    assert {z % 1024 for z in zfs} >= {0, 1, 1023} and any((z + 1) % 44100 == 0 for z in zfs)
    assert {len(h) % 2 for h in host} == {0, 1}
    want, _ = definition(gpu, R44, None, pays, host, zfs)
    got, fused = run(gpu, R44, None, pays, host, zfs)
    assert fused == 1
    assert_equal(got, want, "44.1 kHz")
    assert not np.array_equal(got[1], got[7])               # one input, two offsets and payloads
    # the watermark is there: the output is not the input
    assert not np.array_equal(got[0], host[0])


def batch_rate(gpu, rate):
    if rate == R48:
        shared = pcm16(gpu, 200, 2 * R48 + 5)
        host = [shared] * 5 + [pcm16(gpu, 201, 13001), pcm16(gpu, 202, 60000, silence=(10000, 9000)), pcm16(gpu, 203, 30001)]
        zfs = [3 * 1024 + 17] * 5 + [0, HOUR48, 7 * R48 - 1]
        pays = payloads(5, seed=32)
        return pays + pays[:3], host, zfs
    frame = 1024 * rate // 44100
    host = [pcm16(gpu, 210 + rate // 1000 + i, n) for i, n in enumerate([13001, rate + 1, 2 * rate + 5, 20000])]
    return payloads(4, seed=33), host, [0, rate - 1, 3 * frame + 17, 10 * rate - 10]


@pytest.mark.parametrize("rate", [R48, 32000, 22050])
def test_segments_at_a_rate_equal_the_definition(gpu, rate):
    pays, host, zfs = batch_rate(gpu, rate)
    assert len(host) == (8 if rate == R48 else 4)
    want, _ = definition(gpu, rate, None, pays, host, zfs)
    got, fused = run(gpu, rate, None, pays, host, zfs)
    assert fused == 1
    assert_equal(got, want, f"{rate} Hz")
    if rate == R48:
        assert not np.array_equal(got[0], got[1])           # five subscribers of one segment: five payloads


# ---- 3: loud material -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [R44, R48])
def test_loud_material_ramps_and_saturates(gpu, rate):
    lengths, zfs = [2 * rate + 5, 13001, rate + 1, 30000], [rate - 1, 3 * 1024 + 17, 0, 5 * rate - 20]
    host = [pcm16(gpu, 300 + i, n, level=LOUD) for i, n in enumerate(lengths)]
    pays = payloads(2, seed=34) * 2
    limited, g_limited = definition(gpu, rate, None, pays, host, zfs)
    got, fused = run(gpu, rate, None, pays, host, zfs)
    assert fused == 1
    assert_equal(got, limited, f"loud, {rate} Hz")
    gpu.ctx.set_params(test_no_limiter=1)
    try:
        plain, g_plain = definition(gpu, rate, None, pays, host, zfs)
        got_plain, fused = run(gpu, rate, None, pays, host, zfs)
    finally:
        gpu.ctx.set_params()
    assert fused == 1
    assert_equal(got_plain, plain, f"loud, no limiter, {rate} Hz")
    for i in range(4):
        # the case cannot pass emptily: the DEFINITION's outputs have the ramp (every limiter block of the segment is scaled down) ...
        assert np.abs(g_plain[i]).max() > 1.0 and np.abs(g_limited[i]).max() <= 0.99 + 1e-6
        assert np.abs(limited[i].astype(np.int32)).max() <= 32440
        first = zfs[i] // rate
        for b in range(first, (zfs[i] + lengths[i] - 1) // rate + 1):
            lo, hi = max(b * rate - zfs[i], 0), min((b + 1) * rate - zfs[i], lengths[i])
            assert not np.array_equal(g_limited[i][lo:hi], g_plain[i][lo:hi]), (i, b)
        # ... and both rails of the encode
        assert (plain[i] == 32767).any() and (plain[i] == -32768).any()


# ---- 4: a key per segment -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [R44, R48])
def test_a_key_per_segment(gpu, rate):
    awm = gpu.awm
    lengths, zfs = [13001, 20000, 30001, 13000, 50001, 20000], [1024 * 3 + 1, 0, rate - 1, 1024 * 7, 3 * rate + 11, 1024 * 5 + 1023]
    host = [pcm16(gpu, 400 + i, n) for i, n in enumerate(lengths)]
    keys = [None, awm.test_key(7), awm.test_key(9), awm.test_key(7), None, awm.test_key(9)]
    pays = [payloads(3, seed=35)[i % 3] for i in (0, 1, 2, 1, 0, 0)]
    want, _ = definition(gpu, rate, keys, pays, host, zfs, per_key=True)
    got, fused = run(gpu, rate, keys, pays, host, zfs, per_key=True)
    assert fused == 1
    assert_equal(got, want, f"keys, {rate} Hz")
    # all keys equal: the one-key call
    same = [awm.test_key(7)] * 6
    one, fused_one = run(gpu, rate, awm.test_key(7), pays, host, zfs)
    all_equal, fused_equal = run(gpu, rate, same, pays, host, zfs, per_key=True)
    assert fused_one == fused_equal == 1
    assert_equal(all_equal, one, "equal keys")
    assert_equal(one, definition(gpu, rate, awm.test_key(7), pays, host, zfs)[0], "one key")
    assert not np.array_equal(one[0], got[0])


# ---- 5: alignment and the fallbacks ---------------------------------------------------------------------------------------------------------
def small_batch(gpu, rate, ch=2, n=4):
    lengths, zfs = [13001, 20000, 13003, 30002][:n], [1024 * 3 + 1, rate - 1, 0, 2 * rate + 100][:n]
    host = [pcm16(gpu, 500 + ch + i, m, ch) for i, m in enumerate(lengths)]
    return payloads(3, seed=36)[:n] + payloads(3, seed=36)[:max(0, n - 3)], host, zfs


@pytest.mark.parametrize("rate", [R44, R48])
def test_pointers_off_the_16_byte_grid_stay_fused(gpu, rate):
    """4, 8 and 12 bytes off the grid, inputs and outputs differently: every peel (3, 2, 1 frames) and, with the odd lengths, every tail"""
    pays, host, zfs = small_batch(gpu, rate)
    want = cached(("small", rate, 2), lambda: definition(gpu, rate, None, pays, host, zfs)[0])
    got, fused = run(gpu, rate, None, pays, host, zfs, in_off=[4, 8, 12, 0], out_off=[12, 4, 8, 4])
    assert fused == 1
    assert_equal(got, want, f"4-byte aligned, {rate} Hz")


@pytest.mark.parametrize("rate", [R44, R48])
@pytest.mark.parametrize("what", ["input on 2 bytes", "output on 2 bytes", "single segment", "not batched"])
def test_stereo_fallbacks(gpu, rate, what):
    n = 1 if what == "single segment" else 4
    pays, host, zfs = small_batch(gpu, rate, n=n)
    want = cached(("small", rate, 2), lambda: definition(gpu, rate, None, *small_batch(gpu, rate))[0])[:n]
    in_off = [0, 0, 2, 0][:n] if what == "input on 2 bytes" else None
    out_off = [0, 6, 0, 0][:n] if what == "output on 2 bytes" else None
    if what == "not batched":
        gpu.awm.lib.awm_debug_set_add_batched(0)
    try:
        got, fused = run(gpu, rate, None, pays, host, zfs, in_off=in_off, out_off=out_off)
    finally:
        gpu.awm.lib.awm_debug_set_add_batched(2)
    assert fused == 0
    assert_equal(got, want, f"{what}, {rate} Hz")


@pytest.mark.parametrize("rate", [R44, R48])
@pytest.mark.parametrize("ch", [1, 3])
def test_other_channel_counts_fall_back(gpu, rate, ch):
    pays, host, zfs = small_batch(gpu, rate, ch=ch, n=3)
    want, _ = definition(gpu, rate, None, pays, host, zfs)
    got, fused = run(gpu, rate, None, pays, host, zfs, out_off=[2, 0, 6])
    assert fused == 0
    assert_equal(got, want, f"{ch} channels, {rate} Hz")
    # awm_ctx_trim gives the fallback's workspace back: the call after it has to allocate the decoded and the watermarked copy of the
    # longest segment again (awm_debug_alloc_bytes sums what the library's buffers asked for over the process's life)
    lib = gpu.awm.lib

    def allocated():
        before = lib.awm_debug_alloc_bytes()
        again, _ = run(gpu, rate, None, pays, host, zfs)
        assert_equal(again, want, "again")
        return lib.awm_debug_alloc_bytes() - before
    warm = allocated()
    assert lib.awm_ctx_trim(gpu.ctx._h) == 0
    assert allocated() - warm >= 2 * max(h.size for h in host) * 4


# ---- 6: the context's parameters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [R44, R48])
@pytest.mark.parametrize("params", [dict(test_no_limiter=1), dict(frames_per_bit=3), dict(mix=False), dict(water_delta=0.03)],
                         ids=["no_limiter", "frames_per_bit3", "linear", "water_delta"])
def test_parameters_of_the_context(gpu, rate, params):
    pays, host, zfs = small_batch(gpu, rate)
    default = cached(("small", rate, 2), lambda: definition(gpu, rate, None, pays, host, zfs)[0])
    gpu.ctx.set_params(**params)
    try:
        want, _ = definition(gpu, rate, None, pays, host, zfs)
        got, fused = run(gpu, rate, None, pays, host, zfs)
    finally:
        gpu.ctx.set_params()
    assert fused == 1
    assert_equal(got, want, f"{params}, {rate} Hz")
    if "test_no_limiter" not in params:                     # (quiet material: the limiter has nothing to do there)
        assert not np.array_equal(want[3], default[3])


# ---- 7: launches ----------------------------------------------------------------------------------------------------------------------------
def launch_counts(gpu, rate, n_segments):
    lib, ctx = gpu.awm.lib, gpu.ctx
    lib.awm_prof_name.restype = C.c_char_p
    pool = pcm16(gpu, 600, 13000 + 37 * 32)
    host = [pool[:13000 + 37 * i] for i in range(n_segments)]
    host = [np.ascontiguousarray(h) for h in host]
    zfs = [[0, 1115, 278000, rate - 1, 7 * 1024][i % 5] for i in range(n_segments)]
    pays = payloads(n_segments, seed=37)
    arena, ins, outs = placed(gpu, host)
    ctx.synchronize()
    lib.awm_prof_enable(ctx._h, 1)
    try:
        lib.awm_prof_reset(ctx._h)
        ctx.add_watermark_segments_s16(None, pays, ins, zfs, outs, sample_rate=rate)
        ctx.synchronize()
        counts = {}
        for i in range(lib.awm_prof_count()):
            launches = C.c_long()
            assert lib.awm_prof_read(ctx._h, i, None, C.byref(launches), None) == 0
            counts[lib.awm_prof_name(i).decode()] = launches.value
    finally:
        lib.awm_prof_enable(ctx._h, 0)
    assert gpu.awm.add_segments_fused_in_use() == 1
    arena.check()
    want, _ = definition(gpu, rate, None, pays[:2], host[:2], zfs[:2])
    assert_equal([o.cpu().numpy() for o in outs[:2]], want, f"{n_segments} segments, {rate} Hz")
    return counts


@pytest.mark.parametrize("rate", [R44, R48])
def test_launches_do_not_depend_on_the_number_of_segments(gpu, rate):
    few, many = launch_counts(gpu, rate, 4), launch_counts(gpu, rate, 32)
    assert few == many
    assert few["pcm_decode_kernel"] == 0 and few["pcm_encode_kernel"] == 0
    assert few["limit_encode_s16_kernel"] == 1 and few["add_mix_kernel"] == 1 and few["payload_table_kernel"] == 1
    assert few["segment_gather_s16_kernel"] == (1 if rate == R44 else 0)
    assert few["resample_kernel"] == (0 if rate == R44 else 2)
    # the float call, for comparison, does not touch the new scopes
    pays, host, zfs = small_batch(gpu, rate)
    gpu.awm.lib.awm_prof_enable(gpu.ctx._h, 1)
    try:
        gpu.awm.lib.awm_prof_reset(gpu.ctx._h)
        definition(gpu, rate, None, pays, host, zfs)
        n = {}
        for i in range(gpu.awm.lib.awm_prof_count()):
            launches = C.c_long()
            gpu.awm.lib.awm_prof_read(gpu.ctx._h, i, None, C.byref(launches), None)
            n[gpu.awm.lib.awm_prof_name(i).decode()] = launches.value
    finally:
        gpu.awm.lib.awm_prof_enable(gpu.ctx._h, 0)
    assert n["pcm_decode_kernel"] == 4 and n["pcm_encode_kernel"] == 4
    assert n["limit_encode_s16_kernel"] == 0 and n["segment_gather_s16_kernel"] == 0


# ---- 8: refusals, nothing written -----------------------------------------------------------------------------------------------------------
ERR_ARG = -3


def raw_call(gpu, rate, key, pays, zfs, in_ptrs, out_ptrs, frames, ch=2, per_key=False):
    lib = gpu.awm.lib
    n = len(frames)
    fn = lib.awm_add_watermark_segments_keys_rate_s16_d if per_key else lib.awm_add_watermark_segments_rate_s16_d
    rc = fn(gpu.ctx._h, key, n, (C.c_char_p * n)(*[p.encode() for p in pays]), (C.c_size_t * n)(*zfs), (C.c_void_p * n)(*in_ptrs),
            (C.c_void_p * n)(*out_ptrs), (C.c_size_t * n)(*frames), ch, rate)
    gpu.ctx.synchronize()
    return rc, lib.awm_last_error().decode()


def refusal_batch(gpu):
    lengths, zfs = [13001, 13000, 13003], [1023, 1115, R48 - 1]
    host = [pcm16(gpu, 700 + i, n) for i, n in enumerate(lengths)]
    arena, ins, outs = placed(gpu, host)
    return arena, payloads(3, seed=38), host, zfs, ins, outs, lengths


def nothing_written(arena, outs):
    arena.check()
    return all(arena.untouched(o) for o in outs)


@pytest.mark.parametrize("rate", [R44, R48])
def test_refusals_write_nothing(gpu, rate):
    arena, pays, host, zfs, ins, outs, frames = refusal_batch(gpu)
    i_ptr, o_ptr = [x.data_ptr() for x in ins], [o.data_ptr() for o in outs]
    key = bytes(16)

    def refused(match, **kw):
        args = dict(rate=rate, key=key, pays=pays, zfs=zfs, in_ptrs=i_ptr, out_ptrs=o_ptr, frames=frames)
        args.update(kw)
        rc, err = raw_call(gpu, **args)
        assert rc == ERR_ARG and match in err, (kw, rc, err)
        assert nothing_written(arena, outs), kw

    refused("odd address at index 1", in_ptrs=[i_ptr[0], i_ptr[1] + 1, i_ptr[2]])
    refused("odd address at index 2", out_ptrs=[o_ptr[0], o_ptr[1], o_ptr[2] + 1])
    refused("null pointer at index 1", in_ptrs=[i_ptr[0], None, i_ptr[2]])
    refused("null pointer at index 0", out_ptrs=[None, o_ptr[1], o_ptr[2]])
    # an output that begins on the last int16 value of an input; two outputs that share one value
    refused("overlaps", out_ptrs=[o_ptr[0], i_ptr[0] + (2 * frames[0] - 1) * 2, o_ptr[2]])
    refused("overlaps", out_ptrs=[o_ptr[0], o_ptr[0] + (2 * frames[0] - 1) * 2, o_ptr[2]], frames=[frames[0], 8, frames[2]])
    refused("index 2", pays=[pays[0], pays[1], "xyz"])
    refused("fixed-ratio", rate=44101)
    refused("sample rate", rate=0)
    refused("sample rate", rate=-48000)
    refused("bad argument", key=None, per_key=True)
    if rate != R44:
        refused("segment 1 is not below 2^40", zfs=[zfs[0], 2 ** 40 - 5000, zfs[2]])
    gpu.ctx.snr_begin()
    try:
        refused("SNR")
    finally:
        gpu.ctx.snr_end()
    # ... and the same arguments are taken once nothing is wrong with them
    rc, err = raw_call(gpu, rate, key, pays, zfs, i_ptr, o_ptr, frames)
    assert rc == 0, err
    arena.check()
    assert_equal([o.cpu().numpy() for o in outs], definition(gpu, rate, None, pays, host, zfs)[0], "after the refusals")


@pytest.mark.parametrize("rate", [R44, R48])
def test_buffers_that_touch_and_empty_segments(gpu, rate):
    """the overlap sweep works on bytes of int16: an output that begins where an input ends is accepted (a sweep on 4-byte values would
    see an overlap); empty segments and n_segments == 0 return 0"""
    t = gpu.torch
    n = 13001
    x = pcm16(gpu, 710, n)
    room = t.zeros(4 * n + 64, dtype=t.int16, device="cuda")
    room[:2 * n] = t.from_numpy(x).cuda().reshape(-1)
    i_ptr = room.data_ptr()
    o_ptr = [i_ptr + 2 * n * 2, i_ptr + 2 * n * 2 + 2 * 5000 * 2]          # behind the input, back to back: 5000 and 8001 frames
    pays = payloads(2, seed=39)
    rc, err = raw_call(gpu, rate, bytes(16), pays, [1023, 1023 + 5000], [i_ptr, i_ptr + 2 * 5000 * 2], o_ptr, [5000, n - 5000])
    assert rc == 0, err
    want, _ = definition(gpu, rate, None, pays, [x[:5000], x[5000:]], [1023, 1023 + 5000])
    got = room[2 * n:4 * n].cpu().numpy().reshape(-1, 2)
    assert_equal([got[:5000], got[5000:]], want, "back to back")
    assert not room[4 * n:].any()
    lib = gpu.awm.lib
    assert lib.awm_add_watermark_segments_rate_s16_d(gpu.ctx._h, bytes(16), 0, None, None, None, None, None, 2, rate) == 0
    assert lib.awm_add_watermark_segments_keys_rate_s16_d(gpu.ctx._h, None, 0, None, None, None, None, None, 2, rate) == 0
    rc, err = raw_call(gpu, rate, bytes(16), pays, [5, 7], [None, None], [None, None], [0, 0])
    assert rc == 0, err
    # an empty segment beside one with samples
    out = t.full((5000, 2), 77, dtype=t.int16, device="cuda")
    rc, err = raw_call(gpu, rate, bytes(16), pays, [1023, 9], [i_ptr, None], [out.data_ptr(), None], [5000, 0])
    assert rc == 0, err
    assert np.array_equal(out.cpu().numpy(), want[0])
