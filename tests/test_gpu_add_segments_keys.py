"""A batch of stream segments with a KEY EACH (awm_add_watermark_segments_keys_d / _rate_d): the templates of many
keys built on the device in one launch (K16t), K16p choosing a template per table, and the fused segment paths behind them.

Every comparison is bit for bit.  K16t's templates are held to the host's (awm_tab_frame_mod_template) entry for entry, the tables K16p
expands from them to awm_tab_frame_mod byte for byte; the outputs to the tile stream with that segment's key and payload (torch.equal),
which its own tests pin to the compiled reference, or to the one-key call, which is the function's definition.  The device functions run
on the same values in the same order: there is no tolerance to choose.  Only the comparison with the compiled reference itself has bars,
the ones tests/test_gpu_add_segments.py applies to that comparison.

Segment material, lengths and offsets are those of tests/test_gpu_add_segments.py (MIXED) and, at 48 kHz, the small cases of
tests/test_gpu_add_segments_rate.py; expected tensors are computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import _placement as P

pytestmark = pytest.mark.gpu

SR = 44100
N = 1024
TILE = 128
ERR_ARG = -3
BLOCK = 2226

# tests/test_gpu_add_segments.py's lengths, offsets and MIXED list: 24 (length, zero_frames)
LENGTHS = [0, 1, 1023, 1024, 1025, 3 * N + 17, 2 * SR + 5, 200000]
OFFSETS = [0, 1, 1023, 1024, 3 * N + 17, SR - 1, SR, 10 * SR - 10]
WRAP = 249 * N                       # frame 249 of the stream: table row 4451, the next frame takes row 0
SECOND = (2 * BLOCK + 7) * N         # seven frames into the second pair of watermark blocks
MIXED = ([(LENGTHS[i], OFFSETS[i]) for i in range(8)] + [(LENGTHS[i], OFFSETS[(i + 3) % 8]) for i in range(8)]
         + [(200000, 1), (2 * SR + 5, SR - 1), (1025, 10 * SR - 10), (4 * N + 100, WRAP), (200000, WRAP), (200000, SECOND), (1024, SECOND),
            (0, 1023)])
R48 = 48000
FAR = 3600 * R48 + 12345             # tests/test_gpu_add_segments_rate.py's offset an hour into the stream
STRIDE = (2 * BLOCK * 81 + 15) // 16 * 16              # entries of a template: the table's and the zeros up to a multiple of 16

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
    g.keys = [None, awm.test_key(7), bytes(range(16))]

    def noise(seed, n, ch=2):
        def make():
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed)
            x = torch.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=torch.float32)
            return ((x * 2 - 1) * 0.98).contiguous()
        return cached(("noise", seed, n, ch), make)
    g.noise = noise

    def expected(key, payload, x, seed, zero_frames, tag="default"):
        """the tile stream's output for the segment with that key (shared: keyed by what it depends on)"""
        def make():
            if x.shape[0] == 0:
                return x.clone()
            return ctx.add_watermark_tiles(key, payload, x, TILE, zero_frames=zero_frames)
        return cached(("stream", key, payload, seed, tuple(x.shape), zero_frames, tag), make)
    g.expected = expected
    yield g
    _CACHE.clear()
    awm.lib.awm_debug_set_add_batched(2)
    awm.lib.awm_debug_set_key_tables_on_device(1)
    awm.set_params()
    ctx.set_params()
    ctx.close()


def batch(gpu, cases, n_payloads=6, n_keys=3, ch=2, seed0=100):
    """segment i of a list of (length, zero_frames): noise of seed seed0 + i, key i mod n_keys, payload i mod n_payloads"""
    pays = payloads(n_payloads)
    segs = [gpu.noise(seed0 + i, n, ch) for i, (n, _) in enumerate(cases)]
    return ([gpu.keys[i % n_keys] for i in range(len(cases))], [pays[i % n_payloads] for i in range(len(cases))], segs,
            [zf for _, zf in cases])


def check_against_stream(gpu, keys, pays, segs, zfs, outs, seed0=100, tag="default"):
    for i, (k, p, x, zf, o) in enumerate(zip(keys, pays, segs, zfs, outs)):
        assert o.shape == x.shape
        assert gpu.torch.equal(o, gpu.expected(k, p, x, seed0 + i, zf, tag)), f"segment {i}: {x.shape[0]} samples at zero_frames {zf}"


# ---- 1. K16t alone -------------------------------------------------------------------------------------------------------------------
def host_template(gpu, key):
    return cached(("template", key), lambda: gpu.awm.frame_mod_template(key).reshape(-1))


def check_templates(gpu, keys):
    got = gpu.ctx.key_templates(keys)
    assert got.shape == (len(keys), STRIDE) and got.dtype == np.int16
    for i, key in enumerate(keys):
        want = host_template(gpu, key)
        assert want.size == 2 * BLOCK * 81
        assert np.array_equal(got[i, :want.size], want), f"key {i}"
        assert not got[i, want.size:].any(), f"key {i}: the padding is not zero"
    return got


@pytest.mark.parametrize("which", ["one", "three", "twice"])
def test_key_templates_equal_the_host_templates(gpu, which):
    k = gpu.keys
    got = check_templates(gpu, {"one": [k[1]], "three": k, "twice": [k[2], k[0], k[2]]}[which])
    if which == "three":
        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
        # the format: KEEP / UP / DOWN of the sync bands as values, 4 + 2 k + s for coded bit k < 858, the same names in A and B
        a, b = got[1, :BLOCK * 81], got[1, BLOCK * 81:2 * BLOCK * 81]
        assert set(np.unique(a)) == {0, 1, 2} | set(range(4, 4 + 2 * 858))
        assert np.array_equal(a[a >= 4], b[b >= 4]) and np.array_equal(a >= 4, b >= 4)
        assert np.array_equal(a[(a == 1) | (a == 2)], 3 - b[(b == 1) | (b == 2)])
    if which == "twice":
        assert np.array_equal(got[0], got[2])


def test_key_templates_one_more_than_a_launch(gpu):
    """257 keys: the second launch builds one key into slot 0"""
    keys = [gpu.awm.test_key(1000 + i) for i in range(257)]
    check_templates(gpu, keys)


# ---- 2. K16t + K16p ------------------------------------------------------------------------------------------------------------------
def test_key_payload_tables_equal_the_host_tables(gpu):
    k, p = gpu.keys, payloads(3, seed=13)
    pairs = [(k[0], p[0]), (k[0], p[1]),                     # two payloads under one key
             (k[1], p[0]),                                   # one payload under two keys
             (k[2], p[2]), (k[0], p[0]),                     # a repeated pair
             (k[1], "a5"), (k[2], p[1])]                     # the short payload
    assert len(pairs) == 7
    got = gpu.ctx.key_payload_tables([a for a, _ in pairs], [b for _, b in pairs])
    assert got.shape == (7, 2, BLOCK, 81)
    for i, (key, pay) in enumerate(pairs):
        want = np.zeros((2, BLOCK, 81), np.int8)
        assert gpu.awm.lib.awm_tab_frame_mod(gpu.awm.key_bytes(key), pay.encode(), want.ctypes.data) == want.size
        assert np.array_equal(got[i], want), f"pair {i}"
    assert np.array_equal(got[0], got[4]) and not np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])


def test_the_table_helpers_refuse_another_geometry(gpu):
    gpu.ctx.set_params(frames_per_bit=3)
    try:
        for call in (lambda: gpu.ctx.key_templates(gpu.keys), lambda: gpu.ctx.key_payload_tables(gpu.keys[:2], payloads(2))):
            with pytest.raises(gpu.awm.AwmError, match=r"rc=-3"):
                call()
    finally:
        gpu.ctx.set_params()


# ---- 3. the batch --------------------------------------------------------------------------------------------------------------------
def fused_mixed(gpu):
    def make():
        keys, pays, segs, zfs = batch(gpu, MIXED)
        before = [s.clone() for s in segs]
        outs = gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs)
        gpu.ctx.synchronize()
        fused = gpu.awm.add_segments_fused_in_use()
        assert all(gpu.torch.equal(a, b) for a, b in zip(before, segs)), "an input buffer was written to"
        return outs, fused
    return cached("fused mixed", make)


def test_segments_with_a_key_each_equal_the_stream_path(gpu):
    keys, pays, segs, zfs = batch(gpu, MIXED)
    assert len(segs) == 24 and len(set(pays)) == 6 and len(set(keys)) == 3 and len(set(zip(keys, pays))) == 6
    outs, fused = fused_mixed(gpu)
    assert fused == 1
    check_against_stream(gpu, keys, pays, segs, zfs, outs)
    # the key reaches the table: the same segment, payload and offset under another key is another output
    assert keys[15] != keys[16] and segs[15].shape[0] == 200000
    assert not gpu.torch.equal(outs[15], gpu.expected(keys[16], pays[15], segs[15], 115, zfs[15]))


# ---- 4. one key for all segments IS the one-key function -----------------------------------------------------------------------------
def test_one_key_for_all_segments(gpu):
    _, pays, segs, zfs = batch(gpu, MIXED)
    key = gpu.keys[1]
    want = gpu.ctx.add_watermark_segments(key, pays, segs, zfs)
    got = gpu.ctx.add_watermark_segments_keys([key] * len(segs), pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    assert all(gpu.torch.equal(a, b) for a, b in zip(got, want))
    assert not gpu.torch.equal(got[15], fused_mixed(gpu)[0][15])


# ---- 5. at 48 kHz --------------------------------------------------------------------------------------------------------------------
# shorter than a resampler window, than a 44.1 kHz frame (1115 samples), than a limiter block (48000); one far into the stream
CASES48 = [(17, 1), (1023, 1116), (5000, R48 + 50), (3000, FAR), (R48 + 1, R48 - 1), (1115, 3)]


def test_segments_with_a_key_each_at_48_khz(gpu):
    t = gpu.torch
    keys, pays, segs, zfs = batch(gpu, CASES48, n_payloads=3, n_keys=2, seed0=800)
    # one input for two keys, same payload and offset: segments 6 and 7 alias segment 4
    keys, pays, segs, zfs = keys + gpu.keys[:2], pays + [pays[4]] * 2, segs + [segs[4]] * 2, zfs + [zfs[4]] * 2
    before = [s.clone() for s in segs]
    outs = gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs, sample_rate=R48)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    assert all(t.equal(a, b) for a, b in zip(before, segs)), "an input buffer was written to"
    for key in gpu.keys[:2]:
        mine = [i for i in range(len(segs)) if keys[i] == key]
        assert len(mine) == 4
        want = gpu.ctx.add_watermark_segments(key, [pays[i] for i in mine], [segs[i] for i in mine], [zfs[i] for i in mine], sample_rate=R48)
        gpu.ctx.synchronize()
        for i, w in zip(mine, want):
            assert t.equal(outs[i], w), f"segment {i}: {segs[i].shape[0]} samples at zero_frames {zfs[i]}"
    assert not t.equal(outs[6], outs[7]) and t.equal(outs[4], outs[6])


# ---- 6. other geometries: the host's templates, the fused path -----------------------------------------------------------------------
@pytest.mark.parametrize("params", [dict(frames_per_bit=3), dict(mix=False)], ids=["frames_per_bit3", "linear"])
def test_segments_with_parameters_of_the_context(gpu, params):
    cases = [(3 * N + 17, 1023), (2 * SR + 5, WRAP), (40000, (2 * (510 + 3 * 858) - 251) * N + 5), (1025, SR)]
    tag = tuple(params.items())
    gpu.ctx.set_params(**params)
    try:
        keys, pays, segs, zfs = batch(gpu, cases, n_payloads=2, seed0=340)
        outs = gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 1
        check_against_stream(gpu, keys, pays, segs, zfs, outs, seed0=340, tag=tag)
    finally:
        gpu.ctx.set_params()
    assert not gpu.torch.equal(outs[1], gpu.expected(keys[1], pays[1], segs[1], 341, zfs[1]))


# ---- 7. fallbacks: the same tensors --------------------------------------------------------------------------------------------------
FALLBACK_INDEX = [4, 17, 9, 16, 19]                  # of MIXED, as in tests/test_gpu_add_segments.py; keys 1, 2, 0, 1, 1


def fallback_batch(gpu):
    keys, pays, segs, zfs = batch(gpu, MIXED)
    pick = lambda v: [v[i] for i in FALLBACK_INDEX]
    return pick(keys), pick(pays), pick(segs), pick(zfs)


def check_fallback(gpu, keys, pays, segs, zfs, outs):
    for j, i in enumerate(FALLBACK_INDEX):
        assert gpu.torch.equal(outs[j], gpu.expected(keys[j], pays[j], segs[j], 100 + i, zfs[j])), f"segment {i}"


def test_mono_falls_back(gpu):
    cases = [(3 * N + 17, 1023), (2 * SR + 5, SR - 1), (1025, N), (0, 5)]
    keys, pays, segs, zfs = batch(gpu, cases, n_payloads=2, ch=1, seed0=401)
    outs = gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    check_against_stream(gpu, keys, pays, segs, zfs, outs, seed0=401)


def test_a_misaligned_pointer_falls_back(gpu):
    t = gpu.torch
    keys, pays, segs, zfs = fallback_batch(gpu)
    n = segs[1].shape[0]
    room = t.empty(2 * n + 1, dtype=t.float32, device="cuda")
    shifted = room[1:].view(n, 2)                      # four bytes off the allocation's grid
    shifted.copy_(segs[1])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    outs = gpu.ctx.add_watermark_segments_keys(keys, pays, [segs[0], shifted] + segs[2:], zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    check_fallback(gpu, keys, pays, segs, zfs, outs)


def test_a_single_segment_falls_back(gpu):
    keys, pays, segs, zfs = fallback_batch(gpu)
    outs = gpu.ctx.add_watermark_segments_keys(keys[1:2], pays[1:2], segs[1:2], zfs[1:2])
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    assert gpu.torch.equal(outs[0], gpu.expected(keys[1], pays[1], segs[1], 100 + FALLBACK_INDEX[1], zfs[1]))


def test_the_batched_switch_falls_back(gpu):
    keys, pays, segs, zfs = fallback_batch(gpu)
    gpu.awm.lib.awm_debug_set_add_batched(0)
    try:
        outs = gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 0
    finally:
        gpu.awm.lib.awm_debug_set_add_batched(2)
    check_fallback(gpu, keys, pays, segs, zfs, outs)


def test_templates_from_the_host_give_the_same_tensors(gpu):
    keys, pays, segs, zfs = fallback_batch(gpu)
    gpu.awm.lib.awm_debug_set_key_tables_on_device(0)
    try:
        outs = gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs)
        gpu.ctx.synchronize()
        assert gpu.awm.add_segments_fused_in_use() == 1
    finally:
        gpu.awm.lib.awm_debug_set_key_tables_on_device(1)
    check_fallback(gpu, keys, pays, segs, zfs, outs)
    outs = gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    check_fallback(gpu, keys, pays, segs, zfs, outs)


# ---- 8. group edges ------------------------------------------------------------------------------------------------------------------
def tiny_batch(gpu, keys, pays, seed):
    """a segment of 1024 samples per (key, payload), cut from one buffer on 16-byte starts, on the frame grid"""
    pool = gpu.noise(seed, 8192)
    n = len(keys)
    segs = [pool[2 * (i * 7 % 3000):2 * (i * 7 % 3000) + N] for i in range(n)]
    assert all(s.data_ptr() % 16 == 0 and s.is_contiguous() for s in segs[:8])
    return segs, [(i * 5 % 300) * N for i in range(n)]


def spot_check(gpu, keys, pays, segs, zfs, outs, spots):
    for i in spots:
        want = gpu.ctx.add_watermark_segments(keys[i], [pays[i]] * 2, [segs[i]] * 2, [zfs[i]] * 2)
        gpu.ctx.synchronize()
        assert gpu.torch.equal(want[0], want[1])
        assert gpu.torch.equal(outs[i], want[0]), f"segment {i}"


def test_more_pairs_than_a_table_group(gpu):
    """1025 distinct pairs over 3 keys: ordered by key, table 1024 is the last pair of the third key's run -- the second group's K16p reads
    a template the first group's K16t left behind"""
    n = 1025
    pays = payloads(n, seed=31)
    keys = [gpu.keys[i % 3] for i in range(n)]
    order = sorted(range(n), key=lambda i: (gpu.awm.key_bytes(keys[i]), i))
    assert order[1024] == 1022 and keys[order[1023]] == keys[order[1024]] == gpu.keys[2]
    segs, zfs = tiny_batch(gpu, keys, pays, 900)
    outs = gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    spot_check(gpu, keys, pays, segs, zfs, outs, [0, 1, 2, 512, order[1022], order[1023], order[1024], 1024])


def test_more_keys_than_a_template_launch(gpu):
    """260 distinct keys: K16t in a launch of 256 and one of 4"""
    n = 260
    keys = [gpu.awm.test_key(2000 + i) for i in range(n)]
    pays = [payloads(4, seed=32)[i % 4] for i in range(n)]
    segs, zfs = tiny_batch(gpu, keys, pays, 901)
    outs = gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 1
    spot_check(gpu, keys, pays, segs, zfs, outs, [0, 1, 128, 200, 255, 256, 257, 259])


# ---- 9. launch counts ----------------------------------------------------------------------------------------------------------------
def scope_counts(gpu, n_segments):
    awm, ctx = gpu.awm, gpu.ctx
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    cases = [(5000 + 37 * (i % 24), [0, 1023, WRAP, SR - 1, 7 * N][i % 5]) for i in range(n_segments)]
    keys, pays, segs, zfs = batch(gpu, cases, seed0=500)
    assert len(set(keys)) == 3 and len(set(zip(keys, pays))) == 6
    ctx.synchronize()
    lib.awm_prof_enable(ctx._h, 1)
    try:
        lib.awm_prof_reset(ctx._h)
        outs = ctx.add_watermark_segments_keys(keys, pays, segs, zfs)
        ctx.synchronize()
        assert awm.add_segments_fused_in_use() == 1
        counts = {}
        for i in range(lib.awm_prof_count()):
            launches = C.c_long()
            assert lib.awm_prof_read(ctx._h, i, None, C.byref(launches), None) == 0
            counts[lib.awm_prof_name(i).decode()] = launches.value
    finally:
        lib.awm_prof_enable(ctx._h, 0)
    check_against_stream(gpu, keys[:3], pays[:3], segs[:3], zfs[:3], outs[:3], seed0=500)
    return counts


def test_launches_do_not_depend_on_the_number_of_segments(gpu):
    few, many = scope_counts(gpu, 24), scope_counts(gpu, 96)
    for scope in ("key_template_kernel", "payload_table_kernel", "add_mix_kernel", "limiter_kernel"):
        assert few[scope] == many[scope] == 1, scope
    assert few["frame_mod_table_kernel"] == many["frame_mod_table_kernel"] == 0
    assert few == many


# ---- 10. refusals: AWM_ERR_ARG, nothing enqueued -------------------------------------------------------------------------------------
def refusal_batch(gpu):
    t = gpu.torch
    keys, pays, segs, zfs = batch(gpu, [(3 * N + 17, 1023), (5000, N), (1025, SR - 1)], n_payloads=3, seed0=600)
    outs = [t.full_like(s, float("nan")) for s in segs]
    return keys, pays, segs, zfs, outs


def untouched(gpu, outs):
    gpu.ctx.synchronize()
    return all(bool(gpu.torch.isnan(o).all()) for o in outs)


def raw_call(gpu, keys, pays, segs, zfs, outs, rate=None, **null):
    n = len(segs)
    hexes = (C.c_char_p * n)(*[p.encode() if p is not None else None for p in pays])
    zf = (C.c_size_t * n)(*zfs)
    src = (C.c_void_p * n)(*[s.data_ptr() if s is not None else None for s in segs])
    dst = (C.c_void_p * n)(*[o.data_ptr() if o is not None else None for o in outs])
    frames = (C.c_size_t * n)(*[3 * N + 17, 5000, 1025][:n])
    args = dict(key_bytes=b"".join(gpu.awm.key_bytes(k) for k in keys), hexes=hexes, zf=zf, src=src, dst=dst, frames=frames)
    args.update(null)
    a = (gpu.ctx._h, args["key_bytes"], n, args["hexes"], args["zf"], args["src"], args["dst"], args["frames"], 2)
    if rate is not None:
        return gpu.awm.lib.awm_add_watermark_segments_keys_rate_d(*a, rate)
    return gpu.awm.lib.awm_add_watermark_segments_keys_d(*a)


@pytest.mark.parametrize("rate", [None, R48], ids=["44100", "48000"])
def test_refuses_a_null_pointer(gpu, rate):
    keys, pays, segs, zfs, outs = refusal_batch(gpu)
    for name in ("key_bytes", "hexes", "zf", "src", "dst", "frames"):
        assert raw_call(gpu, keys, pays, segs, zfs, outs, rate, **{name: None}) == ERR_ARG, name
    assert raw_call(gpu, keys, pays, segs, zfs, [outs[0], None, outs[2]], rate) == ERR_ARG
    assert b"index 1" in gpu.awm.lib.awm_last_error()
    assert raw_call(gpu, keys, pays, [segs[0], segs[1], None], zfs, outs, rate) == ERR_ARG
    assert raw_call(gpu, keys, [pays[0], None, pays[2]], segs, zfs, outs, rate) == ERR_ARG
    assert untouched(gpu, outs)
    assert gpu.awm.lib.awm_add_watermark_segments_keys_d(gpu.ctx._h, None, 0, None, None, None, None, None, 2) == 0


def test_refuses_an_output_that_overlaps(gpu):
    keys, pays, segs, zfs, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match="overlaps"):
        gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs, [outs[0], segs[1], outs[2]])          # an input
    room = gpu.torch.full((4996 + 1025, 2), float("nan"), device="cuda")
    with pytest.raises(gpu.awm.AwmError, match="overlaps"):
        gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs, [outs[0], room[:5000], room[4996:4996 + 1025]])      # another output
    assert untouched(gpu, outs) and bool(gpu.torch.isnan(room).all())


def test_refuses_a_payload_that_does_not_parse(gpu):
    keys, pays, segs, zfs, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match="index 2"):
        gpu.ctx.add_watermark_segments_keys(keys, [pays[0], pays[1], "xyz"], segs, zfs, outs)
    assert untouched(gpu, outs)


def test_refuses_a_call_while_the_snr_meter_is_armed(gpu):
    keys, pays, segs, zfs, outs = refusal_batch(gpu)
    gpu.ctx.snr_begin()
    try:
        with pytest.raises(gpu.awm.AwmError, match="SNR"):
            gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs, outs)
    finally:
        gpu.ctx.snr_end()
    assert untouched(gpu, outs)
    gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs, outs)
    gpu.ctx.synchronize()
    check_against_stream(gpu, keys, pays, segs, zfs, outs, seed0=600)


def test_refuses_a_rate_without_a_table_and_an_offset_beyond_2_to_the_40(gpu):
    keys, pays, segs, zfs, outs = refusal_batch(gpu)
    with pytest.raises(gpu.awm.AwmError, match="fixed-ratio"):
        gpu.ctx.add_watermark_segments_keys(keys, pays, segs, zfs, outs, sample_rate=44101)
    with pytest.raises(gpu.awm.AwmError, match="segment 1 is not below"):
        gpu.ctx.add_watermark_segments_keys(keys, pays, segs, [zfs[0], 2 ** 40 - 5000, zfs[2]], outs, sample_rate=R48)
    assert untouched(gpu, outs)


# ---- 11. against the compiled reference ----------------------------------------------------------------------------------------------
def test_a_segment_against_the_compiled_reference(gpu):
    """segment 7 of the batch (200000 samples, test_key (7), ten seconds in with r != 0) against the reference's own add_stream_watermark with
    that key and zero_frames, under the bars of tests/test_gpu_add_segments.py: PCM RMS < 1e-6, max < 2e-6"""
    import _ref
    if not _ref.available():
        pytest.skip("oracle/_ref is not built")
    index = 7
    keys, pays, segs, zfs = batch(gpu, MIXED)
    outs, _ = fused_mixed(gpu)
    n = segs[index].shape[0]
    assert n >= 2 * SR and keys[index] == gpu.awm.test_key(7) and zfs[index] % N != 0
    ref = _ref.add_at(keys[index], segs[index].cpu().numpy(), 2, pays[index], zfs[index]).reshape(-1, 2)
    assert ref.shape == (n, 2)
    d = outs[index].cpu().numpy().astype(np.float64) - ref
    print("rms %.3g max %.3g" % (np.sqrt((d ** 2).mean()), np.abs(d).max()))
    assert np.sqrt((d ** 2).mean()) < 1e-6 and np.abs(d).max() < 2e-6


# ---- 12. placement -------------------------------------------------------------------------------------------------------------------
def test_buffers_at_four_byte_alignment_between_guards(gpu):
    t = gpu.torch
    keys, pays, segs, zfs = fallback_batch(gpu)
    host = [s.cpu().numpy() for s in segs]
    arena = P.Arena(t, P.need(*[h.nbytes for h in host] * 2), device="cuda")
    ins = [arena.place(h, t.float32, 4 + 8 * (i % 2), name="segment %d in" % i) for i, h in enumerate(host)]
    outs = [arena.place(h.shape, t.float32, 12 - 8 * (i % 2), name="segment %d out" % i) for i, h in enumerate(host)]
    assert all(b.data_ptr() % 8 == 4 for b in ins + outs)
    got = gpu.ctx.add_watermark_segments_keys(keys, pays, ins, zfs, outs)
    gpu.ctx.synchronize()
    assert gpu.awm.add_segments_fused_in_use() == 0
    for o in outs:
        arena.assert_written(o)
    arena.check()
    check_fallback(gpu, keys, pays, segs, zfs, got)
