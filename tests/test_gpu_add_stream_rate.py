"""The tile stream at sample rates other than 44.1 kHz (awm_add_stream_create_rate_at / _payloads_rate_at).

THE DEFINITION every comparison uses, bit for bit (torch.equal): the concatenated output of the object is what awm_add_watermark_d writes
for the concatenated input (zero_frames == 0) and what awm_add_watermark_segments_rate_d writes for the single segment (zero_frames, input)
otherwise -- whole calls on the same context, never the object itself.  The object runs the same device functions on the same values at the
same global indices, so there is no tolerance to choose; only the comparison with the compiled reference has bars, those of
tests/test_gpu_streaming.py (f32: max 4e-6, RMS 1e-6).

The tile is the minimum, 128 frames = 131 072 samples: at 48 kHz no multiple of either resampler's np (131 072 mod 160 = 32, mod 147 = 95)
and no multiple of a limiter block (48 000), so every push carries a remainder and every tile edge lies inside a block.  Every output
tile is copied out of the object before the next push.  Material is seeded noise x 0.98: the limiter is at work in every block."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R48 = 48000
T = 128 * 1024
P48 = 2605056000                     # period of the whole pipeline in zero_frames at 48 kHz (tests/test_gpu_add_segments_rate.py)
FAR = 3600 * R48 + 12345
PAY = "0123456789abcdef0011223344556677"

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def payloads(n, seed=31):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, 16, dtype=np.uint8).tobytes().hex() for _ in range(n)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    ctx = awm.Context(0)
    awm.lib.awm_debug_set_resample_phase(1)
    awm.lib.awm_last_error.restype = C.c_char_p

    class G:
        pass
    g = G()
    g.torch, g.awm, g.ctx = torch, awm, ctx

    def noise(seed, n, ch=2, scale=0.98):
        def make():
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed)
            x = torch.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=torch.float32)
            return ((x * 2 - 1) * scale).contiguous()
        return cached(("noise", seed, n, ch, scale), make)
    g.noise = noise

    def expected(rate, key, payload, x, zero_frames, tag):
        """the definition: a whole call (tag names the material and the parameters in force)"""
        def make():
            if x.shape[0] == 0:
                return x.clone()
            if zero_frames == 0:
                w = ctx.add_watermark(key, payload, x, sample_rate=rate)
            else:
                w = ctx.add_watermark_segments(key, [payload], [x], [zero_frames], sample_rate=rate)[0]
            ctx.synchronize()
            return w.clone()
        return cached(("whole", rate, key, payload, tuple(x.shape), zero_frames, tag), make)
    g.expected = expected
    yield g
    _CACHE.clear()
    ctx.set_params()
    ctx.close()


class Stream:
    """the object, pushed by hand: every finished tile is copied out before the next push"""

    def __init__(self, gpu, pays, ch, rate, tile_frames=128, zero_frames=0, key=None):
        self.gpu, self.P, self.ch, self.tile = gpu, len(pays), ch, tile_frames * 1024
        lib = gpu.awm.lib
        self.h = C.c_void_p()
        hexes = (C.c_char_p * self.P)(*[p.encode() for p in pays])
        rc = lib.awm_add_stream_create_payloads_rate_at(gpu.ctx._h, gpu.awm.key_bytes(key), hexes, self.P, ch, rate, tile_frames, zero_frames,
                                                        C.byref(self.h))
        gpu.awm.binding._check(rc, "awm_add_stream_create_payloads_rate_at")
        assert lib.awm_add_stream_sample_rate(self.h) == rate and lib.awm_add_stream_payloads(self.h) == self.P
        self.tiles = [[] for _ in pays]                       # per payload: the finished tiles
        self.final_after = []                                 # per finished tile: the push (0-based) that returned it
        self.pushes = 0

    def push(self, x, last):
        gpu, lib, t = self.gpu, self.gpu.awm.lib, self.gpu.torch
        esz = 4 * self.ch
        if x.shape[0]:
            gpu.awm.binding._hip_memcpy_dtod(gpu.ctx, lib.awm_add_stream_input(self.h), x.data_ptr(), x.shape[0] * esz)
        done_p, done_n = (C.c_void_p * (3 * self.P))(), (C.c_size_t * 3)()
        k = lib.awm_add_stream_push_payloads(self.h, x.shape[0], int(last), done_p, done_n)
        gpu.awm.binding._check(k, "awm_add_stream_push_payloads")
        assert 0 <= k <= 3
        for i in range(k):
            for p in range(self.P):
                out = t.empty((done_n[i], self.ch) if self.ch > 1 else (done_n[i],), dtype=t.float32, device="cuda")
                gpu.awm.binding._hip_memcpy_dtod(gpu.ctx, out.data_ptr(), done_p[i * self.P + p], done_n[i] * esz)
                self.tiles[p].append(out)
            self.final_after.append(self.pushes)
        self.pushes += 1
        return k

    def run(self, x):
        """all of x, tile by tile; a multiple of the tile ends with an empty last push"""
        pos = 0
        while True:
            got = min(self.tile, x.shape[0] - pos)
            last = got < self.tile
            self.push(x[pos:pos + got], last)
            pos += got
            if last:
                break
        return self.result(x)

    def result(self, x):
        t = self.gpu.torch
        self.gpu.ctx.synchronize()
        # the contract: the tiles have the lengths of the input tiles, and tile t is final no later than the push of tile t + 2
        lens = [o.shape[0] for o in self.tiles[0]]
        n = x.shape[0]
        assert lens == [self.tile] * (n // self.tile) + ([n % self.tile] if n % self.tile else []), lens
        last_push = self.pushes - 1
        assert all(after <= min(i + 2, last_push) for i, after in enumerate(self.final_after)), self.final_after
        return [t.cat(o) if o else x[:0].clone() for o in self.tiles]

    def close(self):
        if self.h:
            self.gpu.awm.lib.awm_add_stream_destroy(self.h)
            self.h = C.c_void_p()


def through_tiles(gpu, pays, x, rate, zero_frames=0, tile_frames=128, key=None):
    s = Stream(gpu, pays, x.shape[1] if x.dim() > 1 else 1, rate, tile_frames, zero_frames, key)
    try:
        return s.run(x)
    finally:
        s.close()


# ---- whole equals tiles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 17, 2 * 18 - 1, T - 1, T, T + 1, 2 * T, 2 * T + 5, 3 * T + 48001])
def test_whole_equals_tiles(gpu, n):
    x = gpu.noise(900, 3 * T + 48001)[:n]
    out = through_tiles(gpu, [PAY], x, R48)[0]
    assert out.shape == x.shape
    assert gpu.torch.equal(out, gpu.expected(R48, None, PAY, x, 0, "noise900"))


def test_the_binding_takes_the_rate(gpu):
    x = gpu.noise(900, 3 * T + 48001)[:2 * T + 5]
    assert gpu.torch.equal(gpu.ctx.add_watermark_tiles(None, PAY, x, sample_rate=R48), gpu.expected(R48, None, PAY, x, 0, "noise900"))
    assert gpu.torch.equal(gpu.ctx.add_watermark_tiles(None, PAY, x, sample_rate=44100), gpu.ctx.add_watermark_tiles(None, PAY, x))


# ---- zero_frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zf", [1, 159, 160, 161, 1115, 47999, 48000, 278000, FAR])
def test_zero_frames(gpu, zf):
    x = gpu.noise(901, 2 * T + 5)
    out = through_tiles(gpu, [PAY], x, R48, zero_frames=zf)[0]
    assert gpu.torch.equal(out, gpu.expected(R48, None, PAY, x, zf, "noise901")), zf


def test_zero_frames_a_period_apart(gpu):
    x = gpu.noise(901, 2 * T + 5)
    a = through_tiles(gpu, [PAY], x, R48, zero_frames=1115)[0]
    b = through_tiles(gpu, [PAY], x, R48, zero_frames=1115 + P48)[0]
    assert gpu.torch.equal(a, b) and gpu.torch.equal(a, gpu.expected(R48, None, PAY, x, 1115, "noise901"))


# ---- other rates and channel counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,ch,tile_frames", [(32000, 2, 128), (96000, 2, 128), (22050, 1, 128), (R48, 3, 128), (176400, 2, 256)])
def test_other_rates_and_channel_counts(gpu, rate, ch, tile_frames):
    x = gpu.noise(902 + ch, 2 * tile_frames * 1024 + 5, ch)
    for zf in (0, 1115):
        out = through_tiles(gpu, [PAY], x, rate, zero_frames=zf, tile_frames=tile_frames)[0]
        assert gpu.torch.equal(out, gpu.expected(rate, None, PAY, x, zf, "noise902")), (rate, ch, zf)


# ---- loud material ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.98, 0.98 * 300])
def test_loud_material(gpu, scale):
    """every block limited; x 300 the stretch of watermark alone in front of the stream exceeds the ceiling too, and the limiter's ramps
    across the tile edges must be the whole call's"""
    x = gpu.noise(905, 2 * T + 5, 2, scale)
    out = through_tiles(gpu, [PAY], x, R48, zero_frames=1115)[0]
    whole = gpu.expected(R48, None, PAY, x, 1115, "noise905 x %g" % scale)
    assert gpu.torch.equal(out, whole)
    assert float(whole.abs().max()) <= 1.0 and float((whole - x).abs().max()) > 0.01        # (the limiter did work)


# ---- parameters ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,key", [("frames_per_bit", dict(frames_per_bit=3), None), ("linear", dict(mix=0), None),
                                         ("no_limiter", dict(test_no_limiter=1), None), ("key", {}, "key3")])
def test_parameters(gpu, name, kw, key):
    key = gpu.awm.test_key(3) if key else None
    x = gpu.noise(906, 2 * T + 5)
    try:
        if kw:
            gpu.ctx.set_params(**kw)
        for zf in (0, 1115):
            out = through_tiles(gpu, [PAY], x, R48, zero_frames=zf, key=key)[0]
            assert gpu.torch.equal(out, gpu.expected(R48, key, PAY, x, zf, "noise906 " + name)), (name, zf)
    finally:
        gpu.ctx.set_params()


# ---- payloads --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,ch,n_payloads", [(R48, 2, 2), (R48, 2, 5), (32000, 1, 3)])
def test_payloads(gpu, rate, ch, n_payloads):
    pays = payloads(n_payloads)
    x = gpu.noise(907, 2 * T + 5, ch)
    for zf in (0, 1115):
        outs = through_tiles(gpu, pays, x, rate, zero_frames=zf)
        for p, o in zip(pays, outs):
            assert gpu.torch.equal(o, through_tiles(gpu, [p], x, rate, zero_frames=zf)[0]), (rate, n_payloads, zf)
            assert gpu.torch.equal(o, gpu.expected(rate, None, p, x, zf, "noise907"))
    assert gpu.torch.equal(gpu.ctx.add_watermark_payloads_tiles(None, pays, x, sample_rate=rate)[-1], gpu.expected(rate, None, pays[-1], x, 0, "noise907"))


# ---- output while input is outstanding -------------------------------------------------------------------------------------------------
def test_output_while_input_is_outstanding(gpu):
    x = gpu.noise(908, 5 * T)
    whole = gpu.expected(R48, None, PAY, x, 0, "noise908")
    s = Stream(gpu, [PAY], 2, R48)
    try:
        returned = [s.push(x[i * T:(i + 1) * T], False) for i in range(3)]
        gpu.ctx.synchronize()
        assert returned[0] == 0 and sum(returned) >= 1        # tile 0 is final no later than the push of tile 2
        assert gpu.torch.equal(s.tiles[0][0], whole[:T])      # final before tiles 3 and 4 are handed over
        s.push(x[3 * T:4 * T], False)
        s.push(x[4 * T:], False)
        s.push(x[:0], True)
        assert gpu.torch.equal(s.result(x)[0], whole)
    finally:
        s.close()


# ---- bounded work and memory -----------------------------------------------------------------------------------------------------------
def test_bounded_work_and_memory(gpu):
    lib, ctx = gpu.awm.lib, gpu.ctx
    lib.awm_prof_name.restype = C.c_char_p
    x = gpu.noise(909, 7 * T)
    gpu.expected(R48, None, PAY, x, 0, "noise909")            # (tables and workspaces of the context exist before the bytes are counted)
    ctx.synchronize()
    before = lib.awm_debug_alloc_bytes()
    s = Stream(gpu, [PAY], 2, R48)
    created = lib.awm_debug_alloc_bytes()
    counts = []
    lib.awm_prof_enable(ctx._h, 1)
    try:
        for i in range(7):
            ctx.synchronize()
            lib.awm_prof_reset(ctx._h)
            s.push(x[i * T:(i + 1) * T], i == 6)
            ctx.synchronize()
            row = {}
            for j in range(lib.awm_prof_count()):
                launches = C.c_long()
                assert lib.awm_prof_read(ctx._h, j, None, C.byref(launches), None) == 0
                if launches.value:
                    row[lib.awm_prof_name(j).decode()] = launches.value
            counts.append(row)
        out = s.result(x)[0]
        assert lib.awm_debug_alloc_bytes() == created
    finally:
        lib.awm_prof_enable(ctx._h, 0)
        s.close()
    assert lib.awm_debug_alloc_bytes() == created
    print("launches per push:", counts)
    assert counts[2] == counts[3] == counts[4] and sum(counts[3].values()) >= 4
    # the header's formula: (3 + 3 P) tiles at the rate + (2 + 2 P) tiles at 44.1 kHz; on top the carry of each buffer (a few thousand
    # samples), and the context's allocator gives every one of the 14 buffers at least 1 MiB and up to half as much again as asked for
    tile_bytes = T * 2 * 4
    formula = 6 * tile_bytes + 4 * tile_bytes * 147 // 160
    print("device bytes of the object: %d (formula %d)" % (created - before, formula))
    assert formula <= created - before <= formula * 3 // 2 + 14 * (1 << 20), (created - before, formula)
    assert gpu.torch.equal(out, gpu.expected(R48, None, PAY, x, 0, "noise909"))


# ---- one test per refusal --------------------------------------------------------------------------------------------------------------
def create(gpu, rate=R48, tile_frames=128, zero_frames=0, pays=(PAY,), ch=2, single=False):
    lib = gpu.awm.lib
    h = C.c_void_p()
    before = lib.awm_debug_alloc_bytes()
    if single:
        rc = lib.awm_add_stream_create_rate_at(gpu.ctx._h, bytes(16), pays[0].encode(), ch, rate, tile_frames, zero_frames, C.byref(h))
    else:
        hexes = (C.c_char_p * max(1, len(pays)))(*[p.encode() for p in pays])
        rc = lib.awm_add_stream_create_payloads_rate_at(gpu.ctx._h, bytes(16), hexes, len(pays), ch, rate, tile_frames, zero_frames, C.byref(h))
    return rc, h, lib.awm_last_error().decode(), lib.awm_debug_alloc_bytes() - before


def refused(gpu, words, **kw):
    for single in (True, False):
        rc, h, err, allocated = create(gpu, single=single, **kw)
        assert rc == -3 and not h.value and allocated == 0, (rc, err)
        assert all(w in err for w in words), err


def test_refuses_a_rate_that_is_not_positive(gpu):
    refused(gpu, ["sample_rate"], rate=0)
    refused(gpu, ["sample_rate"], rate=-48000)


def test_refuses_a_rate_without_fixed_ratio_tables(gpu):
    refused(gpu, ["no fixed-ratio resampler", "44101"], rate=44101)
    refused(gpu, ["no fixed-ratio resampler"], rate=2000)


def test_refuses_a_tile_below_min_tile(gpu):
    refused(gpu, ["min_tile", str(gpu.awm.add_stream_rate_plan(176400)["min_tile"])], rate=176400, tile_frames=128)
    rc, h, _, _ = create(gpu, rate=176400, tile_frames=gpu.awm.add_stream_rate_plan(176400)["min_tile"] // 1024)
    assert rc == 0 and h.value
    gpu.awm.lib.awm_add_stream_destroy(h)


def test_refuses_what_the_44_1_khz_constructors_refuse(gpu):
    refused(gpu, ["128 frames"], tile_frames=127)
    refused(gpu, ["bad argument"], ch=0)
    rc, h, err, allocated = create(gpu, pays=())
    assert rc == -3 and not h.value and allocated == 0 and "0 payloads" in err
    rc, h, err, allocated = create(gpu, pays=(PAY,) * 65)
    assert rc == -3 and not h.value and allocated == 0 and "65 payloads" in err
    rc, h, err, allocated = create(gpu, pays=(PAY, "xyz"))
    assert rc == -3 and not h.value and allocated == 0 and "index 1" in err


def test_refuses_creation_while_the_snr_meter_is_armed(gpu):
    gpu.ctx.snr_begin()
    try:
        refused(gpu, ["SNR meter"])
    finally:
        gpu.ctx.snr_end()


def test_refuses_a_push_while_the_snr_meter_is_armed(gpu):
    x = gpu.noise(910, T)
    s = Stream(gpu, [PAY], 2, R48)
    try:
        gpu.ctx.snr_begin()
        try:
            with pytest.raises(gpu.awm.AwmError, match="SNR meter"):
                s.push(x, False)
        finally:
            gpu.ctx.snr_end()
        assert gpu.torch.equal(s.run(x)[0], gpu.expected(R48, None, PAY, x, 0, "noise910"))      # the refused push left nothing behind
    finally:
        s.close()


def test_refuses_a_push_that_reaches_2_to_the_40(gpu):
    refused(gpu, ["2^40"], zero_frames=1 << 40)
    s = Stream(gpu, [PAY], 2, R48, zero_frames=(1 << 40) - T)
    try:
        with pytest.raises(gpu.awm.AwmError, match=r"2\^40"):
            s.push(gpu.noise(910, T), False)
        assert s.push(gpu.noise(910, T)[:T - 1], True) >= 1
    finally:
        s.close()


def test_refuses_awm_add_stream_push_on_many_payloads_and_tiles_that_break_the_contract(gpu):
    lib = gpu.awm.lib
    x = gpu.noise(910, T)
    s = Stream(gpu, payloads(2), 2, R48)
    try:
        done_p, done_n = (C.c_void_p * 3)(), (C.c_size_t * 3)()
        assert lib.awm_add_stream_push(s.h, 0, 1, done_p, done_n) == -3 and b"2 payloads" in lib.awm_last_error()
        with pytest.raises(gpu.awm.AwmError, match="every tile but the last"):
            s.push(x[:T - 1], False)
        s.push(x, True)
        with pytest.raises(gpu.awm.AwmError, match="nothing may follow"):
            s.push(x[:0], True)
        assert not lib.awm_add_stream_input(s.h)
    finally:
        s.close()


# ---- the compiled reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zf", [0, FAR])
def test_against_the_reference(gpu, zf):
    import _ref
    if not _ref.available():
        pytest.skip("oracle/_ref is not built")
    x = gpu.noise(901, 2 * T + 5)
    out = through_tiles(gpu, [PAY], x, R48, zero_frames=zf)[0]
    ref = (_ref.add_at(None, x.cpu().numpy(), 2, PAY, zf, sample_rate=R48) if zf else _ref.add(None, x.cpu().numpy(), 2, PAY, sample_rate=R48))
    ref = ref.reshape(-1, 2)
    assert ref.shape == tuple(x.shape)
    d = out.cpu().numpy().astype(np.float64) - ref
    print("zero_frames %d: max %.3g rms %.3g" % (zf, np.abs(d).max(), np.sqrt((d ** 2).mean())))
    assert np.abs(d).max() <= 4e-6 and np.sqrt((d ** 2).mean()) < 1e-6
