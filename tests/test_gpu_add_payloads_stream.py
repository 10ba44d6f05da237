"""One input, many payloads through a SPAN of a stream (awm_add_mix_payloads_d, K2m's span form), through the tile stream
(awm_add_stream_create_payloads_at / awm_add_stream_push_payloads) and through files (awm_add_watermark_payloads_file).

Every comparison is bit for bit (torch.equal, filecmp): the fused form runs K2's device functions and expressions in K2's order, and the
single-payload paths compared against are pinned to the oracle and the reference by their own tests -- there is no tolerance to choose.

The shapes are the smallest at which this code can go wrong (table wrap, limiter block boundaries inside frames, ragged tails, tile
boundaries), not the workload.  Inputs are generated on the device; results of the single-payload paths are computed once and shared."""
import ctypes as C
import filecmp
import os
import struct

import numpy as np
import pytest

import _placement as PL

pytestmark = pytest.mark.gpu

SR = 44100
N = 1024
TILE = 128                       # frames of 1024 samples per tile: the smallest an awm_add_stream takes
ERR_ARG, ERR_IO = -3, -5         # AWM_ERR_ARG, AWM_ERR_IO (include/awm_hip.h)
ZERO_FRAMES = [0, 7 * 1024 + 5, 3 * 2226 * 1024 + 77]

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


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
    awm.set_payloads_file_tile(0)
    awm.set_params()
    ctx.close()


# ==== 1. the span kernel through awm_add_mix_payloads_d ===========================================================================
STREAM = 300 * N + 333                                   # crosses the table wrap at frame 250 and six limiter blocks, none at a frame boundary
SPANS = [(0, 37), (37, 1), (38, 212), (250, None)]       # (first frame, frames); the last one is the ragged rest: 50 frames + 333 samples


def mix_spans(gpu, x, tables, limiter=True, offset_frames=0):
    """the stream cut into SPANS, every span one awm_add_mix_payloads_d with halos from its neighbours and block maxima shared across
    the spans, then awm_add_limit_d per output and span; returns the concatenated outputs and the fused flags seen"""
    t, ctx = gpu.torch, gpu.ctx
    n = x.shape[0]
    P = len(tables)
    first_block = offset_frames * N // SR
    n_blocks = (offset_frames * N + n) // SR + 2 - first_block
    bms = None
    if limiter:
        bms = [t.empty(n_blocks, dtype=t.float32, device="cuda") for _ in range(P)]
        for b in bms:
            ctx.add_init_block_max(b)
    flags, pieces = [], [[] for _ in range(P)]
    for f0, nf in SPANS:
        lo = f0 * N
        hi = n if nf is None else (f0 + nf) * N
        span = x[lo:hi].contiguous()
        before = x[lo - N:lo].contiguous() if lo else None
        after = x[hi:hi + N].contiguous() if hi < n else None                     # (the last span: NULL, zeros behind the end)
        assert after is None or after.shape[0] == N
        outs = [t.empty_like(span) for _ in range(P)]
        ctx.add_mix_payloads(span, outs, tables, 0.01, offset_frames + f0, before, after, bms, first_block)
        flags.append(gpu.awm.add_payloads_fused_in_use())
        for p in range(P):
            pieces[p].append((lo, outs[p]))
    if limiter:
        for p in range(P):
            for lo, o in pieces[p]:
                ctx.add_limit(o, offset_frames * N + lo, bms[p], first_block)
    ctx.synchronize()
    return [t.cat([o for _, o in pieces[p]]) for p in range(P)], flags, bms


@pytest.mark.parametrize("n_pay", [2, 4, 5])
@pytest.mark.parametrize("ch", [2, 1, 3])
def test_spans_equal_the_whole_stream(gpu, ch, n_pay):
    x = gpu.noise(40 + ch, STREAM, ch)
    pays = payloads(n_pay)
    tables = [gpu.awm.tab_frame_mod(None, p) for p in pays]
    got, flags, _ = mix_spans(gpu, x, tables)
    assert flags == [1] * len(SPANS)
    for p, pay in enumerate(pays):
        want = cached(("whole", ch, pay), lambda: gpu.ctx.add_watermark(None, pay, x))
        assert gpu.torch.equal(got[p], want), f"output {p} of {n_pay}"
    assert not gpu.torch.equal(got[0], got[1])


def test_spans_below_the_ceiling(gpu):
    """+-0.25: no block maximum above the ceiling, the limiter's pass is the identity"""
    x = gpu.noise(44, STREAM, 2, 0.25)
    pays = payloads(3)
    got, flags, _ = mix_spans(gpu, x, [gpu.awm.tab_frame_mod(None, p) for p in pays])
    assert flags == [1] * len(SPANS)
    for p, pay in enumerate(pays):
        assert gpu.torch.equal(got[p], gpu.ctx.add_watermark(None, pay, x))
        assert float(got[p].abs().max()) < 0.5


@pytest.mark.parametrize("ch", [2, 1])
def test_spans_with_the_toggle_off(gpu, ch):
    x = gpu.noise(40 + ch, STREAM, ch)
    pays = payloads(5)
    tables = [gpu.awm.tab_frame_mod(None, p) for p in pays]
    gpu.awm.set_add_payloads_fused(False)
    try:
        got, flags, _ = mix_spans(gpu, x, tables)
    finally:
        gpu.awm.set_add_payloads_fused(True)
    assert flags == [0] * len(SPANS)
    for p, pay in enumerate(pays):
        assert gpu.torch.equal(got[p], cached(("whole", ch, pay), lambda: gpu.ctx.add_watermark(None, pay, x)))


@pytest.mark.parametrize("ch", [2, 3])
def test_spans_without_limiter(gpu, ch):
    """block_max_d = NULL under test_no_limiter"""
    x = gpu.noise(40 + ch, STREAM, ch)
    pays = payloads(3)
    gpu.awm.set_params(test_no_limiter=True)
    try:
        got, flags, bms = mix_spans(gpu, x, [gpu.awm.tab_frame_mod(None, p) for p in pays], limiter=False)
        assert bms is None and flags == [1] * len(SPANS)
        for p, pay in enumerate(pays):
            assert gpu.torch.equal(got[p], gpu.ctx.add_watermark(None, pay, x))
    finally:
        gpu.awm.set_params()
    assert float(got[0].abs().max()) > 1.0                                            # nothing limited it


@pytest.mark.parametrize("first_block_shift", [0, 1], ids=["first_block_of_the_span", "one_block_later"])
@pytest.mark.parametrize("ch", [2, 1])
def test_span_at_a_stream_offset_equals_add_mix(gpu, ch, first_block_shift):
    """first_frame / first_block from a stream offset (frame 5000: block 116, 4202 + 5000 wraps the table), against awm_add_mix_d with
    the same arguments: the un-limited mix and the block maxima, bit for bit.  With first_block one block later the maxima of the
    span's first block lie in front of the array and are dropped, as K2 drops them."""
    t, ctx = gpu.torch, gpu.ctx
    f0 = 5000
    x = gpu.noise(50 + ch, 90 * N + 77, ch)
    span, before, after = x[N:81 * N].contiguous(), x[:N].contiguous(), x[81 * N:82 * N].contiguous()
    first_block = (f0 * N) // SR + first_block_shift
    n_blocks = 4
    pays = payloads(5)
    tables = [gpu.awm.tab_frame_mod(None, p) for p in pays]
    outs = [t.empty_like(span) for _ in pays]
    bms = [t.empty(n_blocks, dtype=t.float32, device="cuda") for _ in pays]
    for b in bms:
        ctx.add_init_block_max(b)
    ctx.add_mix_payloads(span, outs, tables, 0.01, f0, before, after, bms, first_block)
    assert gpu.awm.add_payloads_fused_in_use() == 1
    for p in range(len(pays)):
        want, bm = t.empty_like(span), t.empty(n_blocks, dtype=t.float32, device="cuda")
        ctx.add_init_block_max(bm)
        ctx.add_mix(span, want, tables[p], 0.01, f0, before, after, bm, first_block)
        ctx.synchronize()
        assert t.equal(outs[p], want), p
        assert t.equal(bms[p], bm), p
        assert float(bm.max()) > 1.0                                                   # maxima above the ceiling were recorded
    assert not t.equal(outs[0], outs[1])


def test_mix_payloads_errors_enqueue_nothing(gpu):
    t, ctx, lib = gpu.torch, gpu.ctx, gpu.awm.lib
    x = gpu.noise(60, 20 * N, 2)
    sentinel = 123.5
    outs = [t.full_like(x, sentinel) for _ in range(3)]
    tables = [gpu.awm.tab_frame_mod(None, p) for p in payloads(3)]
    halo = gpu.noise(61, N, 2)

    def untouched():
        ctx.synchronize()
        return all(bool((o == sentinel).all()) for o in outs)

    with pytest.raises(gpu.awm.AwmError, match="output 1 overlaps the input"):
        ctx.add_mix_payloads(x, [outs[0], x, outs[2]], tables, 0.01, 0, None, None, None)
    with pytest.raises(gpu.awm.AwmError, match="outputs 0 and 2 overlap"):
        ctx.add_mix_payloads(x, [outs[0], outs[1], outs[0]], tables, 0.01, 0, None, None, None)
    big = t.full((21 * N, 2), sentinel, device="cuda")
    with pytest.raises(gpu.awm.AwmError, match="output 2 overlaps a halo"):                # the halo lies inside output 2
        ctx.add_mix_payloads(x, [outs[0], outs[1], big[:20 * N]], tables, 0.01, 1, big[19 * N:20 * N], None, None)
    bm = t.empty(4, dtype=t.float32, device="cuda")
    with pytest.raises(ValueError, match="3 outputs but 2 arrays"):                      # the binding's own checks, before the library
        ctx.add_mix_payloads(x, outs, tables, 0.01, 0, None, None, [bm, bm])
    with pytest.raises(ValueError, match="3 tables but 2 outputs"):
        ctx.add_mix_payloads(x, outs[:2], tables, 0.01, 0, None, None, None)
    assert untouched() and bool((big == sentinel).all())
    # n_payloads == 0 and NULL pointers, straight at the C entry
    out_p = (C.c_void_p * 3)(*[o.data_ptr() for o in outs])
    fm_p = (C.c_void_p * 3)(*[tb.ctypes.data for tb in tables])
    assert lib.awm_add_mix_payloads_d(ctx._h, x.data_ptr(), out_p, 0, 20 * N, 2, fm_p, 0.01, 0, None, None, None, 0, 0) == ERR_ARG
    assert lib.awm_add_mix_payloads_d(ctx._h, None, out_p, 3, 20 * N, 2, fm_p, 0.01, 0, None, None, None, 0, 0) == ERR_ARG
    assert lib.awm_add_mix_payloads_d(ctx._h, x.data_ptr(), None, 3, 20 * N, 2, fm_p, 0.01, 0, None, None, None, 0, 0) == ERR_ARG
    assert lib.awm_add_mix_payloads_d(ctx._h, x.data_ptr(), out_p, 3, 20 * N, 2, None, 0.01, 0, None, None, None, 0, 0) == ERR_ARG
    holes = (C.c_void_p * 3)(outs[0].data_ptr(), None, outs[2].data_ptr())
    assert lib.awm_add_mix_payloads_d(ctx._h, x.data_ptr(), holes, 3, 20 * N, 2, fm_p, 0.01, 0, None, None, None, 0, 0) == ERR_ARG
    assert b"index 1" in lib.awm_last_error()
    assert untouched()
    ctx.add_mix_payloads(x, outs, tables, 0.01, 0, None, halo, None)                 # and the same call goes through once nothing is wrong
    assert not untouched()


def test_mix_payloads_on_placed_buffers(gpu):
    """every buffer of the call at a 4-byte-aligned odd offset between guard zones (tests/_placement.py): same bits as at torch's own
    placement, no guard touched.  5 payloads = two passes; stereo (float4 / float2 stores) and mono."""
    t, ctx = gpu.torch, gpu.ctx
    for ch in (2, 1):
        x = gpu.noise(70 + ch, 60 * N, ch).cpu().numpy()
        lo, hi = 3 * N, 57 * N                                                        # frames 3 .. 56, halos = frames 2 and 57
        span, before, after = x[lo:hi], x[lo - N:lo], x[hi:hi + N]
        pays = payloads(5)
        tables = [gpu.awm.tab_frame_mod(None, p) for p in pays]
        n_blocks = 4
        sizes = [span.nbytes] * 6 + [before.nbytes] * 2 + [4 * n_blocks] * 5
        a = PL.Arena(t, PL.need(*sizes), device="cuda")
        xin = a.place(span, t.float32, 4, name="span in")
        outs = [a.place(span.shape, t.float32, off, name="payload %d out" % k) for k, off in enumerate([12, 4, 8, 0, 12])]
        hb = a.place(before, t.float32, 12, name="halo before")
        ha = a.place(after, t.float32, 4, name="halo after")
        bms = [a.place((n_blocks,), t.float32, off, name="block maxima %d" % k) for k, off in enumerate([4, 8, 12, 4, 0])]
        for b in bms:
            ctx.add_init_block_max(b)
        ctx.add_mix_payloads(xin, outs, tables, 0.01, 3, hb, ha, bms, 0)
        assert gpu.awm.add_payloads_fused_in_use() == 1
        ctx.synchronize()
        d = lambda v: t.from_numpy(np.ascontiguousarray(v)).cuda()
        for k in range(5):
            want, bm = t.empty_like(d(span)), t.empty(n_blocks, dtype=t.float32, device="cuda")
            ctx.add_init_block_max(bm)
            ctx.add_mix(d(span), want, tables[k], 0.01, 3, d(before), d(after), bm, 0)
            ctx.synchronize()
            assert t.equal(outs[k].view(t.int32), want.view(t.int32)), (ch, k)
            assert t.equal(bms[k].view(t.int32), bm.view(t.int32)), (ch, k)
            a.assert_written(outs[k])
        a.check()
        assert t.equal(xin, d(span))                                                  # the input is read only


# ==== 2. the tile stream ============================================================================================================
LENGTHS = [3 * TILE * N + 5 * N + 333, 2 * TILE * N, TILE * N + 1, 700, 0]
LENGTH_IDS = ["3tiles_5frames_333", "2tiles", "1tile_1sample", "700samples", "empty"]


def single_tiles(gpu, key, pay, x, zero_frames, tag):
    return cached(("tiles", tag, tuple(x.shape), key, pay, zero_frames),
                  lambda: gpu.ctx.add_watermark_tiles(key, pay, x, TILE, zero_frames=zero_frames))


def check_tiles(gpu, key, pays, x, zero_frames, tag):
    t = gpu.torch
    outs = gpu.ctx.add_watermark_payloads_tiles(key, pays, x, TILE, zero_frames=zero_frames)
    assert len(outs) == len(pays)
    for p, pay in enumerate(pays):
        assert outs[p].shape == x.shape
        assert t.equal(outs[p], single_tiles(gpu, key, pay, x, zero_frames, tag)), f"output {p} of {len(pays)} differs from the one-payload stream"
        if zero_frames == 0 and x.shape[0]:
            assert t.equal(outs[p], cached(("whole", tag, tuple(x.shape), key, pay), lambda: gpu.ctx.add_watermark(key, pay, x)))
    return outs


@pytest.mark.parametrize("zero_frames", ZERO_FRAMES)
@pytest.mark.parametrize("n", LENGTHS, ids=LENGTH_IDS)
@pytest.mark.parametrize("n_pay", [1, 2, 5])
@pytest.mark.parametrize("ch", [2, 1, 3])
def test_tile_stream_equals_one_payload_streams(gpu, ch, n_pay, n, zero_frames):
    x = gpu.noise(80 + ch, n, ch)
    outs = check_tiles(gpu, None, payloads(n_pay), x, zero_frames, "default")
    if n >= 2 * TILE * N and n_pay > 1:
        assert gpu.awm.add_payloads_fused_in_use() == 1
        assert not gpu.torch.equal(outs[0], outs[1])


def test_tile_stream_below_the_ceiling(gpu):
    x = gpu.noise(84, LENGTHS[0], 2, 0.25)
    outs = check_tiles(gpu, None, payloads(3), x, ZERO_FRAMES[1], "quiet")
    assert max(float(o.abs().max()) for o in outs) < 0.5


@pytest.mark.parametrize("params", [dict(frames_per_bit=3), dict(mix=False)], ids=["frames_per_bit3", "linear"])
def test_tile_stream_parameters_of_the_context(gpu, params):
    gpu.awm.set_params(**params)
    try:
        check_tiles(gpu, None, payloads(3), gpu.noise(82, LENGTHS[0], 2), ZERO_FRAMES[1], tuple(params.items()))
    finally:
        gpu.awm.set_params()


def test_tile_stream_test_key(gpu):
    check_tiles(gpu, gpu.awm.test_key(42), payloads(3), gpu.noise(82, LENGTHS[0], 2), 0, "key42")


def test_tile_stream_with_the_toggle_off(gpu):
    x = gpu.noise(82, LENGTHS[0], 2)
    gpu.awm.set_add_payloads_fused(False)
    try:
        check_tiles(gpu, None, payloads(5), x, ZERO_FRAMES[1], "default")
        assert gpu.awm.add_payloads_fused_in_use() == 0
    finally:
        gpu.awm.set_add_payloads_fused(True)


def test_tile_stream_rejects_bad_use(gpu):
    lib, ctx = gpu.awm.lib, gpu.ctx
    pays = payloads(2)

    def hexes(ps):
        return (C.c_char_p * len(ps))(*[p.encode() for p in ps])
    h = C.c_void_p()
    assert lib.awm_add_stream_payloads(None) == 0
    assert lib.awm_add_stream_create_payloads_at(ctx._h, bytes(16), hexes(pays), 0, 2, TILE, 0, C.byref(h)) == ERR_ARG       # no payloads
    many = payloads(65)
    assert lib.awm_add_stream_create_payloads_at(ctx._h, bytes(16), hexes(many), 65, 2, TILE, 0, C.byref(h)) == ERR_ARG      # more than 64
    assert lib.awm_add_stream_create_payloads_at(ctx._h, bytes(16), hexes(pays), 2, 2, 16, 0, C.byref(h)) == ERR_ARG         # tile below 128
    assert lib.awm_add_stream_create_payloads_at(ctx._h, bytes(16), hexes([pays[0], pays[1], "xyz", pays[0]]), 4, 2, TILE, 0, C.byref(h)) == ERR_ARG
    assert b"index 2" in lib.awm_last_error()
    ctx.snr_begin()
    try:
        assert lib.awm_add_stream_create_payloads_at(ctx._h, bytes(16), hexes(pays), 2, 2, TILE, 0, C.byref(h)) == ERR_ARG   # armed SNR meter
        assert b"SNR" in lib.awm_last_error()
    finally:
        ctx.snr_end()
    assert lib.awm_add_stream_create_payloads_at(ctx._h, bytes(16), hexes(pays), 2, 2, TILE, 0, C.byref(h)) == 0
    try:
        assert lib.awm_add_stream_payloads(h) == 2
        one, k = (C.c_void_p * 3)(), (C.c_size_t * 3)()
        assert lib.awm_add_stream_push(h, 1000, 1, one, k) == ERR_ARG                                                       # the old push, two payloads
        assert b"2 payloads" in lib.awm_last_error()
        p = (C.c_void_p * 6)()
        assert lib.awm_add_stream_push_payloads(h, 1000, 0, p, k) == ERR_ARG                                                # a short tile that is not last
        ctx.snr_begin()
        try:
            assert lib.awm_add_stream_push_payloads(h, 1000, 1, p, k) == ERR_ARG
        finally:
            ctx.snr_end()
        assert lib.awm_add_stream_push_payloads(h, 1000, 1, p, k) == 1 and k[0] == 1000 and p[0] and p[1] and p[0] != p[1]
        assert lib.awm_add_stream_push_payloads(h, 0, 1, p, k) == ERR_ARG                                                   # nothing after the last tile
    finally:
        lib.awm_add_stream_destroy(h)
    # an empty stream: `last` with no samples finishes no tile
    assert lib.awm_add_stream_create_payloads_at(ctx._h, bytes(16), hexes(pays), 2, 2, TILE, 0, C.byref(h)) == 0
    try:
        p, k = (C.c_void_p * 6)(), (C.c_size_t * 3)()
        assert lib.awm_add_stream_push_payloads(h, 0, 1, p, k) == 0
    finally:
        lib.awm_add_stream_destroy(h)
    # a one-payload object takes either push
    assert lib.awm_add_stream_create_payloads_at(ctx._h, bytes(16), hexes(pays[:1]), 1, 2, TILE, 0, C.byref(h)) == 0
    try:
        p, k = (C.c_void_p * 3)(), (C.c_size_t * 3)()
        assert lib.awm_add_stream_payloads(h) == 1
        assert lib.awm_add_stream_push(h, 0, 1, p, k) == 0
    finally:
        lib.awm_add_stream_destroy(h)


# ==== 3. the file level =============================================================================================================
SECONDS = 12                                             # 4.04 tiles of 128 frames
FORMATS = {"wav_s16_stereo": (2, 16, 0, False, True), "raw_s24be_mono": (1, 24, 0, True, False), "raw_f32_3ch": (3, 32, 2, False, False)}


def wav_header(n_bytes, channels, rate, bits):
    return b"RIFF" + struct.pack("<I", 36 + n_bytes) + b"WAVEfmt " \
        + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits) + b"data" + struct.pack("<I", n_bytes)


@pytest.fixture(scope="module")
def files(gpu, tmp_path_factory):
    """the input file of a format (written once) and the file add_watermark_file writes for a payload (once per payload and zero_frames)"""
    root = tmp_path_factory.mktemp("payload_files")

    class F:
        pass
    f = F()
    f.root = root

    def source(fmt, rate=SR):
        ch, bits, enc, big, wav = FORMATS[fmt]

        def make():
            x = gpu.noise(90 + ch, SECONDS * rate, ch)
            pcm = gpu.ctx.pcm_encode(x.reshape(-1), bits, enc, big, True).cpu().numpy().tobytes()
            path = root / ("in_%s_%d.%s" % (fmt, rate, "wav" if wav else "raw"))
            with open(path, "wb") as out:
                out.write((wav_header(len(pcm), ch, rate, bits) if wav else b"") + pcm)
            return path, (None if wav else gpu.awm.binding.RawFormat(ch, rate, bits, enc, int(big)))
        return cached(("source", fmt, rate), make)
    f.source = source

    def single(fmt, pay, zero_frames, rate=SR):
        def make():
            src, rf = source(fmt, rate)
            dst = root / ("single_%s_%d_%s_%s" % (fmt, rate, pay, zero_frames))
            gpu.ctx.add_watermark_file(None, pay, src, dst, rf, rf, zero_frames=zero_frames)
            return dst
        return cached(("single file", fmt, rate, pay, zero_frames), make)
    f.single = single
    return f


@pytest.mark.parametrize("zero_frames", [None, 5000])
@pytest.mark.parametrize("n_pay", [2, 5])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_files_equal_the_one_payload_files(gpu, files, tmp_path, fmt, n_pay, zero_frames):
    pays = payloads(n_pay)
    src, rf = files.source(fmt)
    dsts = [tmp_path / ("out%d" % p) for p in range(n_pay)]
    gpu.awm.set_payloads_file_tile(TILE)
    try:
        gpu.ctx.add_watermark_payloads_file(None, pays, src, dsts, rf, rf, zero_frames=zero_frames)
        assert gpu.awm.add_payloads_fused_in_use() == 1
    finally:
        gpu.awm.set_payloads_file_tile(0)
    for p, pay in enumerate(pays):
        want = files.single(fmt, pay, zero_frames)
        assert os.path.getsize(dsts[p]) == os.path.getsize(src)
        assert filecmp.cmp(dsts[p], want, shallow=False), f"file {p} of {n_pay} differs from add_watermark_file's"
    assert not filecmp.cmp(dsts[0], dsts[1], shallow=False)


def test_files_with_the_automatic_tile(gpu, files, tmp_path):
    """no debug tile: the rule of the header (4096 frames at this size), one tile for the whole file"""
    pays = payloads(3)
    src, rf = files.source("wav_s16_stereo")
    dsts = [tmp_path / ("out%d.wav" % p) for p in range(3)]
    gpu.ctx.add_watermark_payloads_file(None, pays, src, dsts)
    for p, pay in enumerate(pays):
        assert filecmp.cmp(dsts[p], files.single("wav_s16_stereo", pay, None), shallow=False)


def test_files_at_48_khz_go_through_the_loop(gpu, files, tmp_path):
    pays = payloads(2)
    src, rf = files.source("wav_s16_stereo", 48000)
    dsts = [tmp_path / ("out%d.wav" % p) for p in range(2)]
    gpu.awm.set_payloads_file_tile(TILE)
    try:
        gpu.ctx.add_watermark_payloads_file(None, pays, src, dsts)
    finally:
        gpu.awm.set_payloads_file_tile(0)
    for p, pay in enumerate(pays):
        assert filecmp.cmp(dsts[p], files.single("wav_s16_stereo", pay, None, 48000), shallow=False)


def test_files_one_and_no_payload(gpu, files, tmp_path):
    pay = payloads(1)[0]
    src, rf = files.source("raw_s24be_mono")
    dst = tmp_path / "one.raw"
    gpu.ctx.add_watermark_payloads_file(None, [pay], src, [dst], rf, rf)
    assert filecmp.cmp(dst, files.single("raw_s24be_mono", pay, None), shallow=False)
    gpu.ctx.add_watermark_payloads_file(None, [], tmp_path / "does_not_exist.raw", [], rf, rf)          # returns 0 and touches nothing
    assert sorted(os.listdir(tmp_path)) == ["one.raw"]


def test_files_errors_leave_existing_files_alone(gpu, files, tmp_path):
    lib, ctx = gpu.awm.lib, gpu.ctx
    pays = payloads(3)
    src, rf = files.source("wav_s16_stereo")
    keep = tmp_path / "precious.wav"
    keep.write_bytes(b"do not truncate me")
    other = tmp_path / "other.wav"

    def call(in_path, out_paths, ps=pays):
        hexes = (C.c_char_p * len(ps))(*[p.encode() for p in ps])
        paths = (C.c_char_p * len(ps))(*[os.fsencode(o) for o in out_paths])
        return lib.awm_add_watermark_payloads_file(ctx._h, bytes(16), hexes, len(ps), os.fsencode(in_path), paths, None, None)

    assert call(src, [other, keep, keep]) == ERR_ARG                                   # two equal output paths
    assert b"1 and 2" in lib.awm_last_error()
    assert call(keep, [other, tmp_path / "b.wav", keep]) == ERR_ARG                    # an output that is the input
    assert b"output path 2" in lib.awm_last_error()
    assert call(src, [other, tmp_path / "b.wav", keep], [pays[0], "xyz", pays[2]]) == ERR_ARG
    assert b"index 1" in lib.awm_last_error()
    assert lib.awm_add_watermark_payloads_file(ctx._h, bytes(16), None, 3, os.fsencode(src), None, None, None) == ERR_ARG
    assert keep.read_bytes() == b"do not truncate me" and not other.exists() and not (tmp_path / "b.wav").exists()
    assert call(tmp_path / "missing.wav", [other, tmp_path / "b.wav", tmp_path / "c.wav"]) == ERR_IO
    assert not other.exists()
    with pytest.raises(ValueError):                                                     # and the binding refuses before the library is called
        ctx.add_watermark_payloads_file(None, pays, src, [other, keep, keep])
    assert keep.read_bytes() == b"do not truncate me"
