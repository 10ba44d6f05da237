"""Whole streams from and to signed 16-bit PCM (awm_add_mix_s16_d, awm_add_limit_s16_d, awm_add_watermark_s16_d,
awm_add_get_watermark_s16_d).

Everything is held by equality.  With f = pcm_decode of the 16-bit input (float (v) * (1 / 32768), exact) and g = what the float twin
writes for f, every 16-bit call writes value for value what pcm_encode (g, direct16) writes.  So the reference side of every comparison
is the EXISTING float entry point between the existing pcm_decode and pcm_encode -- never the code under test --, float outputs are
compared as int32 views, int16 outputs as integers, pattern lists as whole dicts, and there is no tolerance anywhere in this file.

Shapes.  K2: a frame is 1024 samples (lengths 1, 1023, 1024, 1025, 3 x 1024 + 17), the smallest span is 4 frames (9 x 1024 + 5: three
spans), a limiter block is 44100 samples (46 x 1024 + 77: the boundary lies inside frame 43); the 16-bit fetch has three load forms in
stereo (8-, 4- and 2-byte aligned pairs) and two in mono, so the stream sits at byte offsets 0, 2, 4, 6 and 14 from a 16-byte boundary.
The last pass: a run is 2048 frames, a group 4 stereo frames or 8 mono values from the sink's first 16-byte boundary (sink offsets 0, 2,
4, 8, 12, 14; lengths 1 .. 5 and around 2048 and 44100), at most two limiter blocks per run."""
import numpy as np
import pytest

import _oracle as orc
from _placement import CANARY, Arena, need
from test_gpu_get_rate import ERR_ARG, PAY1, cached, gpu, launches, material      # noqa: F401 (gpu: the fixture)
from test_gpu_get_s16 import to_s16

pytestmark = pytest.mark.gpu

FRAME = 1024
BS = 44100                                       # limiter block at 44.1 kHz
PAD = 2048                                       # values of alternating full scale on either side of a placed stream (4096 bytes)
CONVERT_SCOPES = ("pcm_decode_kernel", "pcm_encode_kernel", "limiter_kernel")
LAST_PASS = "limit_encode_s16_kernel"


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def channels(x):
    return 1 if x.dim() == 1 else x.shape[1]


def decode(gpu, s16):
    t = gpu.torch
    return gpu.ctx.pcm_decode(s16.contiguous().view(-1).view(t.uint8), 16).view(s16.shape)


def encode(gpu, x):
    t = gpu.torch
    return gpu.ctx.pcm_encode(x.contiguous().view(-1), 16, 0, False, True).view(t.int16).view(x.shape)


def place_stream(gpu, arena, s16, offset):
    """the stream in the arena, `offset` bytes behind a 16-byte boundary, between runs of alternating full scale"""
    t = gpu.torch
    host = np.empty(2 * PAD + s16.numel(), np.int16)
    host[0::2], host[1::2] = 32767, -32768
    host[PAD: PAD + s16.numel()] = s16.cpu().numpy().reshape(-1)
    placed = arena.place(host, t.int16, offset)
    stream = placed[PAD: PAD + s16.numel()].view(s16.shape)
    assert stream.data_ptr() % 16 == offset and stream.is_contiguous()
    return stream


def place_out(gpu, arena, shape, offset):
    """an int16 sink in the arena, `offset` bytes behind a 16-byte boundary: canaries inside and around"""
    out = arena.place(shape, gpu.torch.int16, offset)
    assert out.data_ptr() % 16 == offset % 16
    return out


def ceiling(gpu):
    def make():
        bm = gpu.torch.empty(1, dtype=gpu.torch.float32, device="cuda")
        gpu.ctx.add_init_block_max(bm)
        return float(bm[0])
    return cached("ceiling", make)


def fused(gpu):
    return gpu.lib.awm_debug_add_s16_fused_in_use()


def definition(gpu, s16, payload=PAY1, rate=44100, key=None):
    """decode, the float call, encode: what every pipeline call has to write"""
    return encode(gpu, gpu.ctx.add_watermark(key, payload, decode(gpu, s16), sample_rate=rate))


# ---- 1. K2, bit for bit ---------------------------------------------------------------------------------------------------------------
K2_FRAMES = 46 * FRAME + 77
# (first sample, samples, halo before, halo after, block maxima: None | (first_block, n_blocks))
K2_CASES = [(0, n, False, False, (0, 3)) for n in (1, 1023, 1024, 1025, 3 * FRAME + 17, 9 * FRAME + 5, K2_FRAMES)] + [
    (0, 3 * FRAME + 17, False, False, None),                         # no limiter
    (3 * FRAME, 17 * FRAME, True, True, (0, 3)),                     # a span with both halos
    (5 * FRAME, K2_FRAMES - 5 * FRAME, True, False, (0, 3)),         # ... that ends with the stream
    (0, 7 * FRAME, False, True, (0, 3)),                             # ... that begins with it
    (44 * FRAME, K2_FRAMES - 44 * FRAME, True, False, (1, 2)),       # first_frame 44 lies in limiter block 1: first_block 1
    (40 * FRAME, 5 * FRAME, True, True, (1, 2)),                     # the block boundary inside the span, block 0 outside the window
]


def k2_material(gpu, C):
    """16-bit noise with both extremes and whole frames of zeros, its decode, and per case what add_mix writes for the decode"""
    t = gpu.torch

    def make():
        x = gpu.noise(9100 + C, K2_FRAMES, C).clone()
        x[2 * FRAME: 3 * FRAME] = 0
        x[41 * FRAME: 43 * FRAME + 5] = 0
        flat = x.view(-1)
        for k, v in ((0, 1.0), (1, -1.0), (flat.numel() - 1, -1.0), (flat.numel() - 2, 1.0), (5 * FRAME * C, -1.0), (5 * FRAME * C + 1, 1.0)):
            flat[k] = v
        s16, dec = to_s16(gpu, x)
        assert int(s16.min()) == -32768 and int(s16.max()) == 32767
        fm = gpu.awm.tab_frame_mod(None, PAY1)
        refs = []
        for a, n, hb, ha, blocks in K2_CASES:
            out = t.empty((n, C) if C > 1 else (n,), dtype=t.float32, device="cuda")
            out.view(t.int32).fill_(CANARY)
            bm = None
            if blocks:
                bm = t.empty(blocks[1], dtype=t.float32, device="cuda")
                gpu.ctx.add_init_block_max(bm)
            gpu.ctx.add_mix(dec[a: a + n], out, fm, 0.01, a // FRAME, dec[a - FRAME: a].contiguous() if hb else None,
                            dec[a + n: a + n + FRAME].contiguous() if ha else None, bm, first_block=blocks[0] if blocks else 0)
            refs.append((out.view(t.int32).clone(), bm.view(t.int32).clone() if blocks else None))
        gpu.ctx.synchronize()
        # the maxima are worth comparing: the loud material lifts a block above the ceiling
        assert any(r[1] is not None and int((r[1].view(t.float32) > ceiling(gpu)).sum()) > 0 for r in refs)
        return s16, fm, refs
    return cached(("k2", C), make)


@pytest.mark.parametrize("offset", (0, 2, 4, 6, 14))
@pytest.mark.parametrize("C", (2, 1, 3), ids=("stereo", "mono", "three"))
def test_k2_add_mix(gpu, C, offset):
    t = gpu.torch
    s16, fm, refs = k2_material(gpu, C)
    arena = Arena(t, need((2 * PAD + s16.numel()) * 2, *[c[1] * C * 4 for c in K2_CASES], *[16] * len(K2_CASES)), device="cuda")
    stream = place_stream(gpu, arena, s16, offset)
    for (a, n, hb, ha, blocks), (ref_out, ref_bm) in zip(K2_CASES, refs):
        out = arena.place((n, C) if C > 1 else (n,), t.float32, 0)                   # (canaries: a NaN pattern until it is written)
        bm = None
        if blocks:
            bm = arena.place(np.zeros(blocks[1], np.float32), t.float32, 0, output=True)
            gpu.ctx.add_init_block_max(bm)
        span = stream[a: a + n]
        assert span.data_ptr() % 16 == offset                                       # whole frames: the span keeps the stream's load form
        gpu.ctx.add_mix_s16(span, out, fm, 0.01, a // FRAME, stream[a - FRAME: a] if hb else None,
                            stream[a + n: a + n + FRAME] if ha else None, bm, first_block=blocks[0] if blocks else 0)
        what = (C, offset, a, n, hb, ha, blocks)
        assert t.equal(out.view(t.int32), ref_out), what
        if blocks:
            assert t.equal(bm.view(t.int32), ref_bm), what
    gpu.ctx.synchronize()
    arena.check()


# ---- 2. the last pass, value for value ------------------------------------------------------------------------------------------------
LP_FRAMES = 2 * BS + 3
# (first sample, frames, first_block): whole-stream lengths, a run of 2048 frames across a block boundary, a table that begins at block 1
LP_CASES = [(0, n, 0) for n in (1, 2, 3, 4, 5, 2047, 2048, 2049, BS - 1, BS, BS + 1, LP_FRAMES)] + [
    (BS - 1000, 5000, 0), (BS - 2047, 4096, 0), (BS + 500, BS - 600, 1), (2 * BS - 100, 103, 1)]
assert all(a + n <= LP_FRAMES for a, n, _ in LP_CASES)
LP_TABLES = ("true", "unity", "none")


def lp_material(gpu, C):
    """a hand-made mix: block 0 below the ceiling, block 1 above it, block 2 (3 frames) below; values beyond +-1 on both sides; products
    that land on whole integers and just beside them; tiny negative values.  Per case and table: add_limit on a copy + pcm_encode"""
    t = gpu.torch

    def make():
        x = (gpu.noise(9200 + C, LP_FRAMES, C) * 0.4).clone()
        x[BS: 2 * BS] *= 4.0                                                    # up to 1.6: above the ceiling and beyond +-1
        flat = x.view(-1)
        k = np.arange(-40000, 40000, 997, dtype=np.float64) / 32768.0           # v * 32768 whole, saturating at both ends
        special = np.concatenate([k, np.nextafter(k.astype(np.float32), np.float32(2)), np.nextafter(k.astype(np.float32), np.float32(-2)),
                                  [-1e-9, -1e-5, -0.9 / 32768, -0.999999 / 32768, 0.999999 / 32768, -1.0, 1.0, 32767 / 32768, -32767.5 / 32768,
                                   1.7, -1.7, -0.0, 0.0]]).astype(np.float32)
        assert special.size <= 280
        sp = t.from_numpy(special).cuda()
        inner = t.from_numpy(special[np.abs(special) < 0.9]).cuda()             # blocks 0 and 2 stay below the ceiling
        for at in (0, 2049 * C, (BS - 300) * C, flat.numel() - inner.numel()):
            flat[at: at + inner.numel()] = inner
        for at in ((BS + 10) * C, (BS + 4096) * C + 1, (2 * BS - 300) * C):
            flat[at: at + sp.numel()] = sp
        cl = ceiling(gpu)
        frames = x.abs().view(LP_FRAMES, -1).amax(dim=1)
        true = t.full((4,), cl, dtype=t.float32, device="cuda")
        for b in range(3):
            true[b] = max(cl, float(frames[b * BS: (b + 1) * BS].max()))
        # from the float path's maxima: blocks above and below the ceiling
        assert float(true[0]) == cl and float(true[1]) > 1.5 and int(x.max() > 1) and int(x.min() < -1)
        unity = t.full((4,), cl, dtype=t.float32, device="cuda")
        tables = {"true": true, "unity": unity, "none": None}
        refs = {}
        for a, n, fb in LP_CASES:
            for name, bm in tables.items():
                copy = x.clone()
                if bm is not None:
                    gpu.ctx.add_limit(copy[a: a + n], a, bm[fb:], first_block=fb)
                refs[(a, n, fb, name)] = encode(gpu, copy[a: a + n]).clone()
        full = refs[(0, LP_FRAMES, 0, "true")]
        assert int(full.max()) < 32767 and int(refs[(0, LP_FRAMES, 0, "unity")].max()) == 32767 and int(refs[(0, LP_FRAMES, 0, "none")].min()) == -32768
        assert not t.equal(full, refs[(0, LP_FRAMES, 0, "unity")])               # the ramp does something
        return x, tables, refs
    return cached(("lp", C), make)


@pytest.mark.parametrize("offset", (0, 2, 4, 8, 12, 14))
@pytest.mark.parametrize("C", (2, 1, 3), ids=("stereo", "mono", "three"))
def test_last_pass(gpu, C, offset):
    t = gpu.torch
    x, tables, refs = lp_material(gpu, C)
    before = x.view(t.int32).clone()
    arena = Arena(t, need(*[c[1] * C * 2 for c in LP_CASES for _ in LP_TABLES]), device="cuda")
    for a, n, fb in LP_CASES:
        for name in LP_TABLES:
            bm = tables[name]
            out = place_out(gpu, arena, (n, C) if C > 1 else (n,), offset)
            _, counts = launches(gpu, lambda: gpu.ctx.add_limit_s16(x[a: a + n], out, a, bm[fb:] if bm is not None else None, first_block=fb))
            want = refs[(a, n, fb, name)]
            what = (C, offset, a, n, fb, name)
            assert t.equal(out, want), (what, int((out != want).sum()))
            assert counts[LAST_PASS] == 1 and all(counts[s] == 0 for s in CONVERT_SCOPES), (what, counts)
    gpu.ctx.synchronize()
    arena.check()
    assert t.equal(x.view(t.int32), before), "mix_d was modified"


def test_last_pass_stereo_mix_off_8_bytes(gpu):
    """a stereo mix that is only 4-byte aligned takes the per-value form: the same values"""
    t = gpu.torch
    x, tables, refs = lp_material(gpu, 2)
    flat = t.empty(x.numel() + 1, dtype=t.float32, device="cuda")
    flat[1:] = x.view(-1)
    moved = flat[1:].view(x.shape)
    assert moved.data_ptr() % 8 == 4
    for name in LP_TABLES:
        out = t.empty(x.shape, dtype=t.int16, device="cuda")
        gpu.ctx.add_limit_s16(moved, out, 0, tables[name], 0)
        assert t.equal(out, refs[(0, LP_FRAMES, 0, name)]), name


# ---- 3. the pipeline call against the definition ---------------------------------------------------------------------------------------
def programme(gpu, seed, seconds, C, rate=44100):
    """(16-bit stream, its decode): the first second near full scale -- the limiter works --, the second quiet, the rest half scale"""
    def make():
        n = int(seconds * rate)
        x = gpu.noise(seed, n, C).clone()
        x[rate: 2 * rate] *= 0.05
        x[2 * rate:] *= 0.5
        return to_s16(gpu, x)
    return cached(("programme", seed, seconds, C, rate), make)


def pipeline_check(gpu, s16, rate=44100, offset=0, want_fused=1, payload=PAY1):
    """add_watermark_s16 into a guarded sink at the byte offset, from a guarded stream at the same one, against the definition"""
    t = gpu.torch
    want = definition(gpu, s16, payload, rate)
    assert s16.shape[0] < FRAME or not t.equal(want, s16)                   # (the watermark is audible to 16 bits in any whole frame)
    arena = Arena(t, need((2 * PAD + s16.numel()) * 2, s16.numel() * 2), device="cuda")
    stream = place_stream(gpu, arena, s16, offset)
    out = place_out(gpu, arena, tuple(s16.shape), offset)
    _, counts = launches(gpu, lambda: gpu.ctx.add_watermark_s16(None, payload, stream, out, sample_rate=rate))
    assert t.equal(out, want), (rate, offset, int((out != want).sum()))
    assert fused(gpu) == want_fused
    if want_fused:
        assert all(counts[s] == 0 for s in CONVERT_SCOPES) and counts[LAST_PASS] > 0, counts
    else:
        assert counts["pcm_decode_kernel"] == 1 and counts["pcm_encode_kernel"] == 1 and counts[LAST_PASS] == 0, counts
    gpu.ctx.synchronize()
    arena.check()
    assert t.equal(stream, s16), "the input was modified"
    return counts


@pytest.mark.parametrize("C,offset", ((2, 0), (2, 4), (2, 2), (2, 14), (1, 0), (1, 2), (3, 0), (3, 6)),
                         ids=("stereo", "stereo+4", "stereo+2", "stereo+14", "mono", "mono+2", "three", "three+6"))
def test_pipeline_44100(gpu, C, offset):
    s16, dec = programme(gpu, 9300 + C, 3, C)
    # the limiter works in the first second and rests in the second
    g = gpu.ctx.add_watermark(None, PAY1, dec)
    h = g.clone()
    gpu.ctx.add_mix(dec, h, gpu.awm.tab_frame_mod(None, PAY1), 0.01, 0, None, None, None)
    assert not gpu.torch.equal(g[:44100], h[:44100]) and gpu.torch.equal(g[90000:120000], h[90000:120000])
    pipeline_check(gpu, s16, offset=offset)


@pytest.mark.parametrize("n", (0, 1, 1025))
@pytest.mark.parametrize("C", (2, 1))
def test_pipeline_short(gpu, C, n):
    t = gpu.torch
    s16, _ = programme(gpu, 9300 + C, 3, C)
    part = s16[:n].contiguous()
    if n:
        pipeline_check(gpu, part)
        return
    out = t.full((4, C) if C > 1 else (4,), 1234, dtype=t.int16, device="cuda")
    _, counts = launches(gpu, lambda: gpu.lib.awm_add_watermark_s16_d(gpu.ctx._h, bytes(16), PAY1.encode(), part.data_ptr(), out.data_ptr(), 0, C, 44100))
    assert _ == 0 and sum(counts.values()) == 0 and int((out != 1234).sum()) == 0
    assert gpu.lib.awm_add_watermark_s16_d(gpu.ctx._h, bytes(16), PAY1.encode(), None, None, 0, C, 48000) == 0


@pytest.mark.parametrize("rate,C", ((44100, 2), (44100, 3), (48000, 2), (48000, 1)))
def test_pipeline_in_place(gpu, rate, C):
    t = gpu.torch
    s16, _ = programme(gpu, 9310 + C, 3, C, rate)
    want = definition(gpu, s16, PAY1, rate)
    arena = Arena(t, need((2 * PAD + s16.numel()) * 2), device="cuda")
    host = np.empty(2 * PAD + s16.numel(), np.int16)
    host[0::2], host[1::2] = 32767, -32768
    host[PAD: PAD + s16.numel()] = s16.cpu().numpy().reshape(-1)
    flat = arena.place(host, t.int16, 4, output=True)
    buf = flat[PAD: PAD + s16.numel()].view(s16.shape)
    got = gpu.ctx.add_watermark_s16(None, PAY1, buf, buf, sample_rate=rate)
    assert got.data_ptr() == buf.data_ptr() and t.equal(buf, want)
    assert fused(gpu) == (1 if (rate == 44100 or C == 2) else 0)
    # the runs of full scale around the stream are where they were
    assert int((flat[:PAD][0::2] != 32767).sum()) == 0 and int((flat[:PAD][1::2] != -32768).sum()) == 0
    assert int((flat[-PAD:][0::2] != 32767).sum()) == 0 and int((flat[-PAD:][1::2] != -32768).sum()) == 0
    gpu.ctx.synchronize()
    arena.check()


def test_pipeline_no_limiter(gpu):
    s16, _ = programme(gpu, 9302, 3, 2)
    limited = definition(gpu, s16)
    gpu.awm.set_params(test_no_limiter=True)
    try:
        assert not gpu.torch.equal(definition(gpu, s16), limited)
        pipeline_check(gpu, s16)
        s48, _ = programme(gpu, 9321, 3, 2, 48000)
        pipeline_check(gpu, s48, rate=48000)
    finally:
        gpu.awm.set_params()


def test_pipeline_frames_per_bit_3(gpu):
    s16, _ = programme(gpu, 9302, 3, 2)
    default = definition(gpu, s16)
    gpu.awm.set_params(frames_per_bit=3)
    try:
        assert not gpu.torch.equal(definition(gpu, s16), default)
        pipeline_check(gpu, s16)
    finally:
        gpu.awm.set_params()


def test_pipeline_context_parameters(gpu):
    """the context's own water_delta applies as for the float call"""
    s16, _ = programme(gpu, 9302, 3, 2)
    default = definition(gpu, s16)
    gpu.ctx.set_params(water_delta=0.02)
    try:
        assert not gpu.torch.equal(definition(gpu, s16), default)
        pipeline_check(gpu, s16)
    finally:
        gpu.ctx.set_params()


@pytest.mark.parametrize("rate", (48000, 32000))
def test_pipeline_rate_fused(gpu, rate):
    s16, _ = programme(gpu, 9320 + rate // 16000, 3, 2, rate)
    counts = pipeline_check(gpu, s16, rate=rate, offset=4)
    assert counts["resample_s16_kernel"] == 1 and counts["add_mix_kernel"] == 1 and counts["resample_kernel"] == 1, counts


@pytest.mark.parametrize("rate,C,offset", ((48000, 1, 0), (48000, 3, 0), (48000, 2, 2), (44101, 2, 0)), ids=("48k-mono", "48k-three", "48k-stereo+2", "44101"))
def test_pipeline_rate_by_definition(gpu, rate, C, offset):
    lib, h = gpu.lib, gpu.ctx._h
    s16, _ = programme(gpu, 9330 + C, 3, C, rate)
    assert lib.awm_ctx_trim(h) == 0 and lib.awm_debug_lane_add_mix_bytes(h) == 0 and lib.awm_debug_lane_pcm_bytes(h) == 0
    pipeline_check(gpu, s16, rate=rate, offset=offset, want_fused=0)
    assert lib.awm_debug_lane_add_mix_bytes(h) >= s16.numel() * 4 and lib.awm_debug_lane_pcm_bytes(h) >= s16.numel() * 4
    assert lib.awm_ctx_trim(h) == 0 and lib.awm_debug_lane_add_mix_bytes(h) == 0 and lib.awm_debug_lane_pcm_bytes(h) == 0


@pytest.mark.parametrize("rate", (44100, 48000))
def test_pipeline_launch_counts_do_not_grow(gpu, rate):
    """the same launches per scope for 3 s and for 30 s; the workspace of the mix goes with awm_ctx_trim"""
    lib, h = gpu.lib, gpu.ctx._h
    short, _ = programme(gpu, 9340, 3, 2, rate)
    long_, _ = programme(gpu, 9341, 30, 2, rate)
    assert lib.awm_ctx_trim(h) == 0
    a = pipeline_check(gpu, short, rate=rate)
    b = pipeline_check(gpu, long_, rate=rate)
    assert a == b, (a, b)
    # the float mix between K2 and the last pass at 44.1 kHz, none at a rate; never a decoded copy of the stream
    assert lib.awm_debug_lane_add_mix_bytes(h) >= (long_.numel() * 4 if rate == 44100 else 0)
    assert lib.awm_debug_lane_add_mix_bytes(h) == 0 or rate == 44100
    assert lib.awm_debug_lane_pcm_bytes(h) == 0
    assert lib.awm_ctx_trim(h) == 0 and lib.awm_debug_lane_add_mix_bytes(h) == 0


# ---- 4. round trip ---------------------------------------------------------------------------------------------------------------------
def test_round_trip(gpu):
    s16, _ = to_s16(gpu, gpu.noise(9400, 65 * 44100, 2) * 0.5)
    out = gpu.ctx.add_watermark_s16(None, PAY1, s16)
    assert fused(gpu) == 1 and out.dtype == gpu.torch.int16 and out.shape == s16.shape
    pats = gpu.ctx.get_watermark_s16(None, out)
    assert any(p["bits"] == PAY1 for p in pats)
    # the anchor outside the library
    ref = orc.get(None, decode(gpu, out).cpu().numpy(), 2)
    assert any(p["bits"] == PAY1 for p in ref)


# ---- 5. watermark, then verify ---------------------------------------------------------------------------------------------------------
def add_get_check(gpu, s16, rate):
    t = gpu.torch
    want_out = gpu.ctx.add_watermark_s16(None, PAY1, s16, sample_rate=rate)
    want = gpu.ctx.get_watermark_s16(None, want_out, sample_rate=rate)
    assert any(p["bits"] == PAY1 for p in want)
    out = t.zeros_like(s16)
    got, counts = launches(gpu, lambda: gpu.ctx.add_get_watermark_s16(None, PAY1, s16, out, sample_rate=rate))
    assert t.equal(out, want_out)
    assert got == want
    assert fused(gpu) == 1 and all(counts[s] == 0 for s in CONVERT_SCOPES), counts
    return counts


def test_add_get_several_chunks(gpu):
    s16, _ = to_s16(gpu, gpu.noise(9500, 8 * 60 * 44100, 2) * 0.5)
    gpu.awm.set_params(chunk_size_min=3.0)
    try:
        chunks = gpu.awm.plan_chunks(s16.shape[0])
        assert len(chunks) >= 3
        counts = add_get_check(gpu, s16, 44100)
        assert counts["sync_db_s16_kernel(approx)"] == len(chunks), (counts, len(chunks))
        assert counts[LAST_PASS] >= 3                                   # a pass per range of chunk ends: the hand-over
        # in place too: the same stream and list
        want_out = gpu.ctx.add_watermark_s16(None, PAY1, s16)
        buf = s16.clone()
        got = gpu.ctx.add_get_watermark_s16(None, PAY1, buf, buf)
        assert gpu.torch.equal(buf, want_out) and got == gpu.ctx.get_watermark_s16(None, want_out)
    finally:
        gpu.awm.set_params()


def test_add_get_48000(gpu):
    s16, _ = to_s16(gpu, gpu.noise(9501, 75 * 48000, 2) * 0.5)
    add_get_check(gpu, s16, 48000)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    t, lib, h = gpu.torch, gpu.lib, gpu.ctx._h
    n, C = 4096, 2
    s16, _ = programme(gpu, 9302, 3, 2)
    arena = Arena(t, need(3 * n * C * 2, n * C * 2, n * C * 4, 64), device="cuda")
    buf = arena.place(np.ascontiguousarray(s16[:3 * n].cpu().numpy()), t.int16, 0, output=True)         # room for overlapping pairs
    kept = buf.clone()
    out = place_out(gpu, arena, (n, C), 0)
    mix = arena.place((n, C), t.float32, 0)
    bm = arena.place(np.full(4, 7.0, np.float32), t.float32, 0, output=True)
    pats = np.full(4096, 0x5a, np.uint8)
    vp = pats.ctypes.data
    key, pay = bytes(16), PAY1.encode()
    fm = gpu.awm.tab_frame_mod(None, PAY1)
    fmp = np.ascontiguousarray(fm, np.int8).ctypes.data
    src, dst = buf.data_ptr(), out.data_ptr()
    frame = 2 * C

    def add(i, o, rate=44100, p=pay, frames=n):
        return lib.awm_add_watermark_s16_d(h, key, p, i, o, frames, C, rate)

    def add_get(i, o, rate=44100, p=pay, frames=n, max_out=8, res=vp):
        return lib.awm_add_get_watermark_s16_d(h, key, p, i, o, frames, C, rate, max_out, res)

    for rate in (44100, 48000):
        calls = [lambda: add(src + 1, dst, rate), lambda: add(src, dst + 1, rate),                       # odd addresses
                 lambda: add(src, src + frame, rate), lambda: add(src + frame, src, rate),               # overlap by all but one frame
                 lambda: add(src, src + (n - 1) * frame, rate), lambda: add(src + (n - 1) * frame, src, rate),     # ... by one frame
                 lambda: add(None, dst, rate), lambda: add(src, None, rate),
                 lambda: add(src, dst, rate, b"not hex"),
                 lambda: lib.awm_add_watermark_s16_d(h, key, pay, src, dst, n, 0, rate),
                 lambda: add_get(src + 1, dst, rate), lambda: add_get(src, src + frame, rate), lambda: add_get(src + frame, src, rate),
                 lambda: add_get(None, dst, rate), lambda: add_get(src, dst, rate, b"not hex"),
                 lambda: add_get(src, dst, rate, max_out=8, res=None)]
        for k, call in enumerate(calls):
            rc, counts = launches(gpu, call)
            assert rc == ERR_ARG and sum(counts.values()) == 0, (rate, k, rc, counts)
            assert lib.awm_last_error()
    for call in (lambda: add(src, dst, -1), lambda: add(src, dst, 0), lambda: add(src, dst, 44100 * 300), lambda: add_get(src, dst, -1)):
        rc, counts = launches(gpu, call)
        assert rc == ERR_ARG and sum(counts.values()) == 0, (rc, counts)
    # the kernel level
    for call in (lambda: lib.awm_add_mix_s16_d(h, src + 1, mix.data_ptr(), n, C, fmp, 0.01, 0, None, None, bm.data_ptr(), 0, 4),
                 lambda: lib.awm_add_mix_s16_d(h, src, mix.data_ptr(), n, C, fmp, 0.01, 0, src + 1, None, bm.data_ptr(), 0, 4),
                 lambda: lib.awm_add_mix_s16_d(h, src, mix.data_ptr(), n, C, fmp, 0.01, 0, None, src + 3, bm.data_ptr(), 0, 4),
                 lambda: lib.awm_add_mix_s16_d(h, None, mix.data_ptr(), n, C, fmp, 0.01, 0, None, None, bm.data_ptr(), 0, 4),
                 lambda: lib.awm_add_mix_s16_d(h, src, None, n, C, fmp, 0.01, 0, None, None, bm.data_ptr(), 0, 4),
                 lambda: lib.awm_add_mix_s16_d(h, src, mix.data_ptr(), n, 0, fmp, 0.01, 0, None, None, bm.data_ptr(), 0, 4),
                 lambda: lib.awm_add_limit_s16_d(h, mix.data_ptr(), dst + 1, n, C, 0, bm.data_ptr(), 0, 4),
                 lambda: lib.awm_add_limit_s16_d(h, None, dst, n, C, 0, bm.data_ptr(), 0, 4),
                 lambda: lib.awm_add_limit_s16_d(h, mix.data_ptr(), None, n, C, 0, bm.data_ptr(), 0, 4),
                 lambda: lib.awm_add_limit_s16_d(h, mix.data_ptr(), dst, n, 0, 0, bm.data_ptr(), 0, 4)):
        rc, counts = launches(gpu, call)
        assert rc == ERR_ARG and sum(counts.values()) == 0, (rc, counts)
    gpu.ctx.synchronize()
    assert arena.untouched(out) and arena.untouched(mix) and t.equal(buf, kept) and int((bm != 7.0).sum()) == 0 and (pats == 0x5a).all()
    arena.check()
    # out_d == pcm_in_d exactly is no overlap
    assert add(src, src) == 0
