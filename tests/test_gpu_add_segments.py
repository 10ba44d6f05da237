"""A batch of stream segments, each with its own offset and payload (awm_add_watermark_segments_d; the reference's HLS mode, hls.cc:279:
add_stream_watermark (key, in, out, bits, zero_frames) per request).

Every comparison is bit for bit (torch.equal) against the tile stream (awm_add_stream_create_at with that payload and zero_frames, fed
the segment), which its own tests pin to the compiled reference: the fused path runs K2's and K3's device functions on the same values
in the same order, with tables that K16p expands on the device from the key's template -- there is no tolerance to choose.  Only the
comparison with the compiled reference itself has bars, the ones tests/test_gpu_streaming.py applies to that comparison.

Material is seeded noise x 0.98: the limiter is at work in every block.  The lengths and offsets are the smallest at which this code can
go wrong (segments inside a frame, frame and limiter block edges, the table wrap, a second watermark block); the expected tensors are
computed once per (payload, segment, offset) and shared."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 44100
N = 1024
TILE = 128
ERR_ARG = -3
BLOCK = 2226

LENGTHS = [0, 1, 1023, 1024, 1025, 3 * N + 17, 2 * SR + 5, 200000]
OFFSETS = [0, 1, 1023, 1024, 3 * N + 17, SR - 1, SR, 10 * SR - 10]
WRAP = 249 * N                       # frame 249 of the stream: table row 4451, the next frame takes row 0
SECOND = (2 * BLOCK + 7) * N         # seven frames into the second pair of watermark blocks

# (length, zero_frames): every length with two of the offsets, the table wrap with three frames and more, the second block pair
MIXED = ([(LENGTHS[i], OFFSETS[i]) for i in range(8)] + [(LENGTHS[i], OFFSETS[(i + 3) % 8]) for i in range(8)]
         + [(200000, 1), (2 * SR + 5, SR - 1), (1025, 10 * SR - 10), (4 * N + 100, WRAP), (200000, WRAP), (200000, SECOND), (1024, SECOND),
            (0, 1023)])
# the same lengths with every segment on the frame grid: nothing is staged
ALIGNED_OFFSETS = [0, N, 3 * N, 43 * N, WRAP, 431 * N, SECOND, 44 * N]
ALIGNED = ([(LENGTHS[i], ALIGNED_OFFSETS[i]) for i in range(8)] + [(LENGTHS[i], ALIGNED_OFFSETS[(i + 3) % 8]) for i in range(8)]
           + [(4 * N + 100, WRAP), (200000, WRAP), (200000, SECOND), (2 * SR + 5, 43 * N)])

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def payloads(n, seed=11):
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

    def expected(key, payload, x, seed, zero_frames, tag="default"):
        """the tile stream's output for the segment (shared: keyed by what it depends on)"""
        def make():
            if x.shape[0] == 0:
                return x.clone()
            return ctx.add_watermark_tiles(key, payload, x, TILE, zero_frames=zero_frames)
        return cached(("stream", key, payload, seed, tuple(x.shape), zero_frames, tag), make)
    g.expected = expected
    yield g
    _CACHE.clear()
    awm.lib.awm_debug_set_add_batched(2)
    ctx.set_params()
    ctx.close()


def batch(gpu, cases, n_payloads=6, ch=2, seed0=100):
    """segments, payloads and offsets of a list of (length, zero_frames): segment i is noise of seed seed0 + i with payload i mod n_payloads"""
    pays = payloads(n_payloads)
    segs = [gpu.noise(seed0 + i, n, ch) for i, (n, _) in enumerate(cases)]
    return [pays[i % n_payloads] for i in range(len(cases))], segs, [zf for _, zf in cases]


def check_against_stream(gpu, key, pays, segs, zfs, outs, seed0=100, tag="default"):
    t = gpu.torch
    for i, (p, x, zf, o) in enumerate(zip(pays, segs, zfs, outs)):
        assert o.shape == x.shape
        assert t.equal(o, gpu.expected(key, p, x, seed0 + i, zf, tag)), f"segment {i}: {x.shape[0]} samples at zero_frames {zf}"


def fused_mixed(gpu):
    def make():
        pays, segs, zfs = batch(gpu, MIXED)
        outs = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
        gpu.ctx.synchronize()
        return outs, gpu.awm.add_segments_fused_in_use()
    return cached("fused mixed", make)


def test_segments_equal_the_stream_path(gpu):
    pays, segs, zfs = batch(gpu, MIXED)
    assert len(segs) == 24 and len(set(pays)) == 6
    outs, fused = fused_mixed(gpu)
    assert fused == 1
    check_against_stream(gpu, None, pays, segs, zfs, outs)
    # the offset and the payload both matter: the same material elsewhere in the stream, or for another subscriber, is another output
    x = segs[15]
    assert not gpu.torch.equal(outs[15], gpu.expected(None, pays[15 % 6], x, 115, zfs[15] + N))
    assert not gpu.torch.equal(outs[15], gpu.expected(None, pays[0], x, 115, zfs[15]))


def test_segments_on_the_frame_grid_are_not_staged(gpu):
    t = gpu.torch
    pays, segs, zfs = batch(gpu, ALIGNED, seed0=200)
    assert all(zf % N == 0 for zf in zfs)
    before = [s.clone() for s in segs]
    outs = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    check_against_stream(gpu, None, pays, segs, zfs, outs, seed0=200)
    assert all(t.equal(a, b) for a, b in zip(before, segs)), "an input buffer was written to"


def test_one_segment_for_five_subscribers(gpu):
    pays = payloads(5, seed=12)
    x = gpu.noise(300, 2 * SR + 5)
    zf = 3 * N + 17
    before = x.clone()
    outs = gpu.ctx.add_watermark_segments(None, pays, [x] * 5, [zf] * 5)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    for p, o in zip(pays, outs):
        assert gpu.torch.equal(o, gpu.expected(None, p, x, 300, zf))
    assert gpu.torch.equal(before, x) and not gpu.torch.equal(outs[0], outs[1])


def test_segments_with_a_test_key(gpu):
    key = gpu.awm.test_key(7)
    cases = [(3 * N + 17, 1023), (2 * SR + 5, WRAP), (1025, SR), (20000, 10 * SR - 10)]
    pays, segs, zfs = batch(gpu, cases, n_payloads=3, seed0=320)
    outs = gpu.ctx.add_watermark_segments(key, pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    check_against_stream(gpu, key, pays, segs, zfs, outs, seed0=320)


@pytest.mark.parametrize("index", [7, 17, 20])
def test_segments_against_the_compiled_reference(gpu, index):
    """three of the segments above (r != 0 ten seconds in, r != 0 one sample before a limiter block edge, the table wrap on the frame grid) against
    the reference's own add_stream_watermark with that zero_frames, under the bars of tests/test_gpu_streaming.py: PCM RMS < 1e-6, max < 2e-6"""
    import _ref
    if not _ref.available():
        pytest.skip("oracle/_ref is not built")
    pays, segs, zfs = batch(gpu, MIXED)
    outs, _ = fused_mixed(gpu)
    n = segs[index].shape[0]
    assert n >= 2 * SR
    ref = _ref.add_at(None, segs[index].cpu().numpy(), 2, pays[index], zfs[index]).reshape(-1, 2)
    assert ref.shape == (n, 2)
    d = outs[index].cpu().numpy().astype(np.float64) - ref
    print("rms %.3g max %.3g" % (np.sqrt((d ** 2).mean()), np.abs(d).max()))
    assert np.sqrt((d ** 2).mean()) < 1e-6 and np.abs(d).max() < 2e-6


@pytest.mark.parametrize("params", [dict(frames_per_bit=3), dict(mix=False)], ids=["frames_per_bit3", "linear"])
def test_segments_with_parameters_of_the_context(gpu, params):
    """a block of 510 + 3 x 858 frames, and --linear: the template, K16p and K2 take the geometry as arguments"""
    cases = [(3 * N + 17, 1023), (2 * SR + 5, WRAP), (40000, (2 * (510 + 3 * 858) - 251) * N + 5), (1025, SR)]
    tag = tuple(params.items())
    gpu.ctx.set_params(**params)
    try:
        pays, segs, zfs = batch(gpu, cases, n_payloads=3, seed0=340)
        outs = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 1
        check_against_stream(gpu, None, pays, segs, zfs, outs, seed0=340, tag=tag)
    finally:
        gpu.ctx.set_params()
    assert not gpu.torch.equal(outs[1], gpu.expected(None, pays[1], segs[1], 341, zfs[1]))


def test_segments_without_the_limiter(gpu):
    cases = [(3 * N + 17, 1023), (2 * SR + 5, SR - 1), (1025, N)]
    gpu.ctx.set_params(test_no_limiter=1)
    try:
        pays, segs, zfs = batch(gpu, cases, n_payloads=2, seed0=360)
        outs = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 1
        check_against_stream(gpu, None, pays, segs, zfs, outs, seed0=360, tag="no limiter")
    finally:
        gpu.ctx.set_params()
    assert float(outs[1].abs().max()) > 1.0


@pytest.mark.parametrize("params", [dict(), dict(frames_per_bit=3)], ids=["default", "frames_per_bit3"])
def test_payload_tables_from_the_template(gpu, params):
    """K16p alone: the tables it expands on the device are the host's tables, byte for byte"""
    block_frames = 510 + 858 * params.get("frames_per_bit", 2)
    pays = payloads(5, seed=13) + ["a5", payloads(5, seed=13)[0]]
    key = gpu.awm.test_key(3)
    gpu.ctx.set_params(**params)
    gpu.awm.set_params(**params)                      # (awm_tab_frame_mod takes the process-wide set)
    try:
        got = gpu.ctx.payload_tables(key, pays, block_frames)
        for p, table in zip(pays, got):
            want = np.zeros((2, block_frames, 81), np.int8)
            assert gpu.awm.lib.awm_tab_frame_mod(gpu.awm.key_bytes(key), p.encode(), want.ctypes.data) == want.size
            assert np.array_equal(table, want), p
    finally:
        gpu.awm.set_params()
        gpu.ctx.set_params()


# ---- everything the fused path does not take goes segment by segment through the tile stream: the same tensors ---------------------
FALLBACK_INDEX = [4, 17, 9, 16, 19]                  # of MIXED: r != 0 and r == 0, one sample, a frame, a few seconds


def fallback_batch(gpu):
    pays, segs, zfs = batch(gpu, MIXED)
    return [pays[i] for i in FALLBACK_INDEX], [segs[i] for i in FALLBACK_INDEX], [zfs[i] for i in FALLBACK_INDEX]


def check_fallback(gpu, pays, segs, zfs, outs):
    for j, i in enumerate(FALLBACK_INDEX):
        assert gpu.torch.equal(outs[j], gpu.expected(None, pays[j], segs[j], 100 + i, zfs[j])), f"segment {i}"


@pytest.mark.parametrize("ch", [1, 3])
def test_other_channel_counts_fall_back(gpu, ch):
    cases = [(3 * N + 17, 1023), (2 * SR + 5, SR - 1), (1025, N), (0, 5)]
    pays, segs, zfs = batch(gpu, cases, n_payloads=2, ch=ch, seed0=400 + ch)
    outs = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    check_against_stream(gpu, None, pays, segs, zfs, outs, seed0=400 + ch)


def test_a_misaligned_pointer_falls_back(gpu):
    t = gpu.torch
    pays, segs, zfs = fallback_batch(gpu)
    n = segs[1].shape[0]
    room = t.empty(2 * n + 1, dtype=t.float32, device="cuda")
    shifted = room[1:].view(n, 2)                      # four bytes off the allocation's grid
    shifted.copy_(segs[1])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    segs = [segs[0], shifted] + segs[2:]
    outs = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    check_fallback(gpu, pays, segs, zfs, outs)


def test_a_single_segment_falls_back(gpu):
    pays, segs, zfs = fallback_batch(gpu)
    outs = gpu.ctx.add_watermark_segments(None, pays[1:2], segs[1:2], zfs[1:2])
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    assert gpu.torch.equal(outs[0], gpu.expected(None, pays[1], segs[1], 100 + FALLBACK_INDEX[1], zfs[1]))


def test_the_toggle_falls_back(gpu):
    pays, segs, zfs = fallback_batch(gpu)
    gpu.awm.lib.awm_debug_set_add_batched(0)
    try:
        outs = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 0
    finally:
        gpu.awm.lib.awm_debug_set_add_batched(2)
    check_fallback(gpu, pays, segs, zfs, outs)
    outs = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    check_fallback(gpu, pays, segs, zfs, outs)


# ---- launch structure ---------------------------------------------------------------------------------------------------------------
def scope_counts(gpu, n_segments):
    awm, ctx = gpu.awm, gpu.ctx
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    cases = [(5000 + 37 * i, [0, 1023, WRAP, SR - 1, 7 * N][i % 5]) for i in range(n_segments)]
    pays, segs, zfs = batch(gpu, cases, n_payloads=n_segments, seed0=500)
    assert len(set(pays)) == n_segments
    ctx.synchronize()
    lib.awm_prof_enable(ctx._h, 1)
    try:
        lib.awm_prof_reset(ctx._h)
        outs = ctx.add_watermark_segments(None, pays, segs, zfs)
        ctx.synchronize()
        assert awm.add_segments_fused_in_use() == 1
        counts = {}
        for i in range(lib.awm_prof_count()):
            launches = C.c_long()
            assert lib.awm_prof_read(ctx._h, i, None, C.byref(launches), None) == 0
            counts[lib.awm_prof_name(i).decode()] = launches.value
    finally:
        lib.awm_prof_enable(ctx._h, 0)
    check_against_stream(gpu, None, pays[:3], segs[:3], zfs[:3], outs[:3], seed0=500)
    return counts


def test_launches_do_not_depend_on_the_number_of_segments(gpu):
    few, many = scope_counts(gpu, 3), scope_counts(gpu, 40)
    for scope in ("payload_table_kernel", "add_mix_kernel", "limiter_kernel"):
        assert few[scope] == many[scope] == 1, scope
    assert few["frame_mod_table_kernel"] == many["frame_mod_table_kernel"] == 0
    assert few == many


# ---- the splits of a call: 4096 segments per launch, 1024 distinct payloads per table group ------------------------------------------
def pool_batch(gpu, n, n_payloads, seed):
    """n short segments cut from one buffer (starts on 16 bytes), offsets in and off the frame grid, segment i with payload i mod n_payloads"""
    pool = gpu.noise(seed, 8192)
    pays = payloads(n_payloads, seed=seed)
    segs, zfs = [], []
    for i in range(n):
        start, length = 2 * (i * 7 % 2000), 600 + i * 13 % 700              # 600 .. 1299 samples: one or two frames, up to three with r
        segs.append(pool[start:start + length])
        zfs.append((i * 5 % 300) * N + (0 if i % 3 else (i * 11 % N)))      # two in three on the frame grid, the others staged
    return [pays[i % n_payloads] for i in range(n)], segs, zfs


def check_split_call(gpu, n, n_payloads, seed, parts, sample):
    """One call that has to be split equals the same segments in calls that are not (bit for bit, every segment), and the segments of
    `sample` -- both sides of the split -- equal the tile stream."""
    t = gpu.torch
    pays, segs, zfs = pool_batch(gpu, n, n_payloads, seed)
    whole = gpu.ctx.add_watermark_segments(None, pays, segs, zfs)
    assert gpu.awm.add_segments_fused_in_use() == 1
    pieces = []
    for a, b in parts:
        assert b - a <= 4096 and len(set(pays[a:b])) <= 1024
        pieces += gpu.ctx.add_watermark_segments(None, pays[a:b], segs[a:b], zfs[a:b])
    gpu.ctx.synchronize()
    assert len(pieces) == n
    bad = [i for i in range(n) if not t.equal(whole[i], pieces[i])]
    assert not bad, f"segments {bad[:8]} differ between the split call and the unsplit ones"
    for i in sample:
        want = gpu.ctx.add_watermark_tiles(None, pays[i], segs[i], TILE, zero_frames=zfs[i])
        assert t.equal(whole[i], want), f"segment {i}: {segs[i].shape[0]} samples at zero_frames {zfs[i]}"


def test_more_payloads_than_a_table_group(gpu):
    """1025 distinct payloads: the tables of payload 1024 are built after the first group's segments are through, into the same area"""
    check_split_call(gpu, 1025, 1025, 700, [(0, 512), (512, 1025)], [0, 3, 1023, 1024])


def test_more_segments_than_a_launch(gpu):
    """4097 segments with 6 payloads: ordered by payload, the 4097th goes into a second launch of every stage"""
    check_split_call(gpu, 4097, 6, 701, [(0, 2048), (2048, 4097)], [0, 3, 4091, 4095, 4096])


def test_payload_tables_refuses_another_geometry(gpu):
    """the library writes the rows of the geometry in force: a block_frames that is not it is refused before a buffer is made"""
    with pytest.raises(ValueError, match="block_frames"):
        gpu.ctx.payload_tables(None, payloads(2), 510 + 858)
    assert gpu.ctx.payload_tables(None, payloads(2)).shape == (2, 2, BLOCK, 81)


def test_an_empty_segment_gets_its_payload_checked(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    empty = segs[0][:0]
    with pytest.raises(gpu.awm.AwmError, match="index 1"):
        gpu.ctx.add_watermark_segments(None, [pays[0], "xyz", pays[2]], [segs[0], empty, segs[2]], zfs, [outs[0], empty.clone(), outs[2]])
    assert untouched(gpu, outs)
    got = gpu.ctx.add_watermark_segments(None, [pays[0], payloads(7)[6], pays[2]], [segs[0], empty, segs[2]], zfs, [outs[0], empty.clone(), outs[2]])
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1 and got[1].shape[0] == 0
    for i in (0, 2):
        assert gpu.torch.equal(got[i], gpu.expected(None, pays[i], segs[i], 600 + i, zfs[i]))


# ---- refusals: AWM_ERR_ARG, nothing enqueued -----------------------------------------------------------------------------------------
def refusal_batch(gpu):
    t = gpu.torch
    pays, segs, zfs = batch(gpu, [(3 * N + 17, 1023), (5000, N), (1025, SR - 1)], n_payloads=3, seed0=600)
    outs = [t.full_like(s, float("nan")) for s in segs]
    return pays, segs, zfs, outs


def untouched(gpu, outs):
    gpu.ctx.synchronize()
    return all(bool(gpu.torch.isnan(o).all()) for o in outs)


def raw_call(gpu, pays, segs, zfs, outs, **null):
    n = len(segs)
    hexes = (C.c_char_p * n)(*[p.encode() if p is not None else None for p in pays])
    zf = (C.c_size_t * n)(*zfs)
    src = (C.c_void_p * n)(*[s.data_ptr() if s is not None else None for s in segs])
    dst = (C.c_void_p * n)(*[o.data_ptr() if o is not None else None for o in outs])
    frames = (C.c_size_t * n)(*[3 * N + 17, 5000, 1025][:n])
    args = dict(hexes=hexes, zf=zf, src=src, dst=dst, frames=frames)
    args.update(null)
    return gpu.awm.lib.awm_add_watermark_segments_d(gpu.ctx._h, bytes(16), n, args["hexes"], args["zf"], args["src"], args["dst"], args["frames"], 2)


def test_refuses_a_null_pointer(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    for name in ("hexes", "zf", "src", "dst", "frames"):
        assert raw_call(gpu, pays, segs, zfs, outs, **{name: None}) == ERR_ARG, name
    assert raw_call(gpu, pays, segs, zfs, [outs[0], None, outs[2]]) == ERR_ARG
    assert b"index 1" in gpu.awm.lib.awm_last_error()
    assert raw_call(gpu, pays, [segs[0], segs[1], None], zfs, outs) == ERR_ARG
    assert raw_call(gpu, [pays[0], None, pays[2]], segs, zfs, outs) == ERR_ARG
    assert untouched(gpu, outs)
    assert gpu.awm.lib.awm_add_watermark_segments_d(gpu.ctx._h, bytes(16), 0, None, None, None, None, None, 2) == 0


def test_refuses_an_output_that_overlaps_an_input(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    n = segs[1].shape[0]
    both = gpu.torch.full((2 * n - 100, 2), float("nan"), device="cuda")
    seg, out = both[:n], both[n - 100:]                 # the output begins inside ANOTHER segment's input
    with pytest.raises(gpu.awm.AwmError, match="overlaps"):
        gpu.ctx.add_watermark_segments(None, pays, [segs[0], seg, segs[2]], zfs, [out[:3 * N + 17], outs[1], outs[2]])
    with pytest.raises(gpu.awm.AwmError, match="overlaps"):
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, [outs[0], segs[1], outs[2]])          # in place
    assert untouched(gpu, outs) and bool(gpu.torch.isnan(both).all())


def test_refuses_outputs_that_overlap(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    room = gpu.torch.full((4996 + 1025, 2), float("nan"), device="cuda")
    with pytest.raises(gpu.awm.AwmError, match="overlaps"):
        gpu.ctx.add_watermark_segments(None, pays, segs, zfs, [outs[0], room[:5000], room[4996:4996 + 1025]])
    with pytest.raises(gpu.awm.AwmError, match="overlaps"):
        gpu.ctx.add_watermark_segments(None, pays[:2], [segs[1], segs[1]], zfs[:2], [outs[1], outs[1]])
    assert untouched(gpu, outs) and bool(gpu.torch.isnan(room).all())


def test_refuses_a_payload_that_does_not_parse(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match="index 2"):
        gpu.ctx.add_watermark_segments(None, [pays[0], pays[1], "xyz"], segs, zfs, outs)
    assert untouched(gpu, outs)


def test_refuses_a_call_while_the_snr_meter_is_armed(gpu):
    pays, segs, zfs, outs = refusal_batch(gpu)
    gpu.ctx.snr_begin()
    try:
        with pytest.raises(gpu.awm.AwmError, match="SNR"):
            gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs)
    finally:
        gpu.ctx.snr_end()
    assert untouched(gpu, outs)
    # ... and afterwards the same call goes through
    gpu.ctx.add_watermark_segments(None, pays, segs, zfs, outs)
    check_against_stream(gpu, None, pays, segs, zfs, outs, seed0=600)
