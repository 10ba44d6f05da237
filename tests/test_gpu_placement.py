"""Every device-pointer entry point of include/awm_hip.h on MISALIGNED, GUARDED caller buffers (tests/_placement.py).

The rest of the GPU suite hands the library fresh torch allocations: 512-byte aligned, with allocator slack behind them.  The kernels
and launchers switch code paths on pointer alignment (float4 / float2 / scalar fetches of K1, K2, K2m, K4; the table + float4 limiter
against the scalar one; paired / LDS-staged resamplers against the generic one; the s16le converters; the batched `add` against the
per-clip launches), and a store or load a few values past a buffer's end would land in slack unseen.  Here every buffer of a call
sits at a chosen byte offset from a 256-byte grid (float buffers 0 / 4 / 8 / 12, byte buffers 0 .. 7; inputs and outputs varied
independently) between guard zones of 64 KiB.  Every case asserts

  (a) bit identity with the same call on fresh torch allocations -- the placement the rest of the suite pins to the oracle.  No
      tolerance: kernels.hh and the kernel comments promise the same operations in the same order on every path;
  (b) all guards intact (outputs: canaries, compared as integers); inputs are guarded by NaNs, so a read past an end that reaches
      the arithmetic breaks (a);
  (c) the oracle at the suite's existing tolerances (oracle results are computed once per entry, length and channel count).

The alignment switch a placement exercises is named where the case is built."""
import json
import os

import numpy as np
import pytest

import _oracle as orc
import _placement as P
from test_gpu_parity import PAY1, PAY2, QUALITY_TOL, RMS_TOL, _np_decode, _np_encode, noise, pkey, rms

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (input byte offset, output byte offset) of float buffers, relative to the 256-byte grid
PAIRS = [(0, 0), (4, 0), (0, 4), (4, 4), (8, 8), (12, 8), (8, 12)]
PAIR_IDS = ["in%d_out%d" % p for p in PAIRS]
IN_OFFSETS = [4, 8, 12]                    # entry points whose results come back to the host: only the input is placed
SPEED_KEY = bytes(range(16))
SPEED_TOL = 2e-6                           # tests/test_gpu_speed.py

_CACHE = {}


def cached(key, fn):
    """oracle results and the results at the aligned placement: once per (entry, length, channels, ...)"""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


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
    g.dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                 # a fresh torch allocation: the aligned placement
    g.arena = lambda *nbytes: P.Arena(torch, P.need(*nbytes), device="cuda")
    yield g
    _CACHE.clear()
    awm.set_params()
    awm.set_speed_params()
    orc.set_params()
    orc.set_speed_params(False, False, -1)
    ctx.close()


def same_bits(a, b):
    """bit for bit (float32 compared as int32: -0.0 != 0.0, a NaN equals only itself)"""
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def full(p):
    return pkey(p) + (p["sync_quality"], p["decode_error"], p["speed"])


def nbytes(*shape):
    return 4 * int(np.prod(shape))


@pytest.fixture(scope="module")
def stream70():
    n = 70 * 44100
    return orc.add(None, noise(41, n, 2), 2, PAY1).reshape(n, 2)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "golden_v1.json")) as f:
        return json.load(f)


# ---- K1: fft_range -- fetch_stereo / fetch_channel: float4 (16-byte aligned), float2 (stereo otherwise; mono at 8), scalar (mono at 4 / 12,
# ---- 3 channels); `start` moves the frame's first sample by a further 77 * C floats.  The complex output is placed too. -----------------
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("start", [0, 77])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_fft_range(gpu, ch, start, pair):
    x = noise(21 + ch, 12000, ch)
    want = cached(("fft_range", ch, start), lambda: orc.fft_range(x, ch, start, 8))
    aligned = cached(("fft_range aligned", ch, start), lambda: gpu.ctx.fft_range(gpu.dev(x), start, 8))
    a = gpu.arena(x.nbytes, nbytes(8, ch, 513, 2))
    xin = a.place(x, gpu.torch.float32, pair[0])
    out = a.place((8, ch, 513, 2), gpu.torch.float32, pair[1])
    got = gpu.ctx.fft_range(xin, start, 8, out=out)
    gpu.torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and out.data_ptr() % 16 == pair[1] and xin.data_ptr() % 16 == pair[0]
    assert same_bits(got, aligned)
    a.check()
    a.assert_written(out)
    assert np.abs(got.cpu().numpy() - want).max() < 1e-6 * np.abs(want).max()
    with pytest.raises(gpu.awm.AwmError):                      # reading past the end is still refused, not read from the guard
        gpu.ctx.fft_range(xin, 12000 - 1000, 1)


# ---- K2 + K3: add_watermark -- K2's fetches as above, its float4 / float2 stores of the stereo output (whatever the alignment of out),
# ---- and launch_limiter: table + float4 form for a 16-byte aligned output, the scalar limiter_kernel over the WHOLE stream otherwise ---
ADD_LENGTHS = [1, 700, 1024, 1025, 3 * 1024 + 2, 5 * 44100 + 1, 20 * 44100 + 13]


def add_input(ch, n):
    return noise(100 + ch + n % 97, n, ch)                     # full scale: the limiter has work to do (asserted below)


def oracle_add(ch, limiter, n):
    def run():
        orc.set_params(test_no_limiter=not limiter)
        try:
            return orc.add(None, add_input(ch, n), ch, PAY1).reshape(n, ch)
        finally:
            orc.set_params()
    return cached(("add", ch, limiter, n), run)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("n", ADD_LENGTHS)
@pytest.mark.parametrize("limiter", [True, False], ids=["limiter", "no_limiter"])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_add_watermark(gpu, ch, limiter, n, pair):
    t = gpu.torch
    x = add_input(ch, n)
    want = oracle_add(ch, limiter, n)
    if limiter and n >= 44100:
        assert np.abs(oracle_add(ch, False, n)).max() > 0.99                   # the limiter path really runs
    gpu.awm.set_params(test_no_limiter=not limiter)
    try:
        aligned = cached(("add aligned", ch, limiter, n), lambda: gpu.ctx.add_watermark(None, PAY1, gpu.dev(x)))
        a = gpu.arena(x.nbytes, x.nbytes)
        xin = a.place(x, t.float32, pair[0])
        out = a.place((n, ch), t.float32, pair[1])
        got = gpu.ctx.add_watermark(None, PAY1, xin, out=out)
        t.cuda.synchronize()
    finally:
        gpu.awm.set_params()
    assert xin.data_ptr() % 16 == pair[0] and out.data_ptr() % 16 == pair[1]
    assert same_bits(got, aligned)
    a.check()
    a.assert_written(out)
    assert same_bits(xin, gpu.dev(x))                                            # the input is read only
    g = got.cpu().numpy()
    assert rms(g, want) < RMS_TOL and np.abs(g - want).max() < 2e-6


# ---- awm_add_mix_d + awm_add_limit_d on spans cut from a longer stream: first_frame / first_sample != 0, halos and block maxima at
# ---- offsets of their own.  The one case where the scalar limiter runs with first_sample != 0 on 1 / 2 channels. ----------------------
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("ch", [2, 1])
def test_add_mix_and_limit_on_placed_spans(gpu, ch, pair):
    t = gpu.torch
    n, split = 12 * 44100 + 321, 200 * 1024
    x = noise(55 + ch, n, ch)
    fm = gpu.awm.tab_frame_mod(None, PAY1)
    whole = cached(("add_d aligned", ch), lambda: gpu.ctx.add_d(gpu.dev(x), fm, 0.01, True))
    want = cached(("add_d", ch), lambda: orc.add(None, x, ch, PAY1).reshape(n, ch))

    def unlimited():
        orc.set_params(test_no_limiter=True)
        try:
            return float(np.abs(orc.add(None, x, ch, PAY1)).max())
        finally:
            orc.set_params()
    assert cached(("add_d peak", ch), unlimited) > 0.99                          # the limiter has work to do: the ramps are not all (1, 0)
    n_blocks = n // 44100 + 2
    halo = nbytes(1024, ch)
    a = gpu.arena(x[:split].nbytes, x[split:].nbytes, x[:split].nbytes, x[split:].nbytes, halo, halo, nbytes(n_blocks))
    in_a = a.place(x[:split], t.float32, pair[0], name="span a in")
    in_b = a.place(x[split:], t.float32, (pair[0] + 8) % 16, name="span b in")
    out_a = a.place((split, ch), t.float32, pair[1], name="span a out")
    out_b = a.place((n - split, ch), t.float32, (pair[1] + 4) % 16, name="span b out")
    halo_after = a.place(x[split:split + 1024], t.float32, (pair[0] + 4) % 16, name="halo after a")
    halo_before = a.place(x[split - 1024:split], t.float32, (pair[0] + 12) % 16, name="halo before b")
    bm = a.place((n_blocks,), t.float32, (pair[1] + 12) % 16, name="block maxima")
    gpu.ctx.add_init_block_max(bm)
    gpu.ctx.add_mix(in_a, out_a, fm, 0.01, 0, None, halo_after, bm)
    gpu.ctx.add_mix(in_b, out_b, fm, 0.01, split // 1024, halo_before, None, bm)
    gpu.ctx.add_limit(out_a, 0, bm)
    gpu.ctx.add_limit(out_b, split, bm)
    t.cuda.synchronize()
    assert same_bits(t.cat([out_a, out_b]), whole)
    a.check()
    a.assert_written(bm)
    got = whole.cpu().numpy()
    assert rms(got, want) < RMS_TOL and np.abs(got - want).max() < 2e-6


# ---- K2m: add_watermark_payloads, 5 payloads = two tile passes; every output at an offset of its own -------------------------------
PAYLOADS = [PAY1, PAY2, "00000000000000000000000000000000", "ffffffffffffffffffffffffffffffff", "0f1e2d3c4b5a69788796a5b4c3d2e1f0"]


@pytest.mark.parametrize("in_off", [0, 4, 8, 12])
@pytest.mark.parametrize("ch", [2, 1])
def test_add_watermark_payloads(gpu, ch, in_off):
    t = gpu.torch
    n = 3 * 44100 + 17
    x = noise(300 + ch, n, ch)
    singles = cached(("payloads aligned", ch), lambda: [gpu.ctx.add_watermark(None, p, gpu.dev(x)) for p in PAYLOADS])
    a = gpu.arena(*[x.nbytes] * 6)
    xin = a.place(x, t.float32, in_off)
    out_offsets = [(in_off + 4 * (k + 1)) % 16 for k in range(3)] + [0, 12]
    outs = [a.place((n, ch), t.float32, o, name="payload %d out" % k) for k, o in enumerate(out_offsets)]
    assert gpu.awm.ADD_PAYLOADS_TILE < len(PAYLOADS)                               # two tile passes
    got = gpu.ctx.add_watermark_payloads(None, PAYLOADS, xin, outs=outs)
    t.cuda.synchronize()
    assert gpu.awm.add_payloads_fused_in_use() == 1
    for k in range(len(PAYLOADS)):
        assert same_bits(got[k], singles[k]), k
        a.assert_written(outs[k])
    a.check()
    for k in (0, 4):                                                              # one output of either pass against the oracle
        want = cached(("payloads", ch, k), lambda: orc.add(None, x, ch, PAYLOADS[k]).reshape(n, ch))
        g = got[k].cpu().numpy()
        assert rms(g, want) < RMS_TOL and np.abs(g - want).max() < 2e-6


# ---- the clip batches of `add`: one launch per stage while every clip pointer is 16-byte aligned (add_clips_batchable), per-clip launches
# ---- for the whole batch as soon as one is not ----------------------------------------------------------------------------------------
BATCH_LENGTHS = [44100 + 1, 30001, 500, 2 * 44100 + 3, 1025, 70001, 9 * 1024 + 7, 3 * 44100 + 777]


@pytest.mark.parametrize("variant", ["all_aligned", "one_input_misaligned", "one_output_misaligned"])
@pytest.mark.parametrize("entry", ["batch", "batch_keys"])
def test_add_watermark_batches(gpu, entry, variant):
    t = gpu.torch
    clips = [noise(2100 + i, n, 2) * (1.6 if i == 3 else 1.0) for i, n in enumerate(BATCH_LENGTHS)]
    keys = [gpu.awm.test_key(1 + i) for i in range(len(clips))] if entry == "batch_keys" else [None] * len(clips)
    one_by_one = cached(("add batch aligned", entry), lambda: [gpu.ctx.add_watermark(k, PAY2, gpu.dev(c)) for k, c in zip(keys, clips)])
    a = gpu.arena(*[c.nbytes for c in clips] * 2)
    in_off = [0] * len(clips)
    out_off = [0] * len(clips)
    if variant == "one_input_misaligned":
        in_off[3] = 4
    if variant == "one_output_misaligned":
        out_off[5] = 8
    ins = [a.place(c, t.float32, o, name="clip %d in" % i) for i, (c, o) in enumerate(zip(clips, in_off))]
    outs = [a.place(c.shape, t.float32, o, name="clip %d out" % i) for i, (c, o) in enumerate(zip(clips, out_off))]
    if entry == "batch_keys":
        got = gpu.ctx.add_watermark_batch_keys(keys, PAY2, ins, outs=outs)
    else:
        got = gpu.ctx.add_watermark_batch(None, PAY2, ins, outs=outs)
    t.cuda.synchronize()
    for i in range(len(clips)):
        assert same_bits(got[i], one_by_one[i]), i
        a.assert_written(outs[i])
    a.check()
    assert float(one_by_one[3].abs().max()) <= 1.0 and not same_bits(one_by_one[3], gpu.dev(clips[3]))
    for i in (0, 3):
        want = cached(("add batch", entry, i), lambda: orc.add(keys[i], clips[i], 2, PAY2).reshape(-1, 2))
        g = got[i].cpu().numpy()
        assert rms(g, want) < RMS_TOL and np.abs(g - want).max() < 2e-6


# ---- awm_add_watermark_d / awm_add_d refuse an output that overlaps the input (three input frames per output frame: a race) -------------
@pytest.mark.parametrize("kind", ["alias", "front", "back", "one_value"])
@pytest.mark.parametrize("entry", ["add_watermark", "add_d"])
@pytest.mark.parametrize("ch", [2, 1])
def test_add_refuses_an_output_that_overlaps_the_input(gpu, ch, entry, kind):
    t = gpu.torch
    n, k = 5000, 1800
    a = gpu.arena(nbytes(2 * n, ch))
    both = a.place((2 * n, ch), t.float32, 4, name="input and output")            # all canaries: nothing may read or write it
    if kind == "alias":
        xin, out = both[:n], both[:n]
    elif kind == "front":                                                         # the output starts inside the input
        xin, out = both[:n], both[k:k + n]
    elif kind == "back":                                                          # the output ends inside the input
        xin, out = both[k:k + n], both[:n]
    else:                                                                         # the last value of the input is the first of the output
        flat = both.view(-1)
        xin, out = flat[:n * ch].view(n, ch), flat[n * ch - 1:2 * n * ch - 1].view(n, ch)
    fm = gpu.awm.tab_frame_mod(None, PAY1)
    with pytest.raises(gpu.awm.AwmError, match=r"rc=-3\).*overlaps the input"):
        if entry == "add_watermark":
            gpu.ctx.add_watermark(None, PAY1, xin, out=out)
        else:
            gpu.ctx.add_d(xin, fm, 0.01, True, out=out)
    t.cuda.synchronize()
    assert a.untouched(both)
    a.check()
    # buffers that only touch are fine: the output right behind the input
    x = noise(77 + ch, n, ch)
    both[:n].copy_(gpu.dev(x))
    if entry == "add_watermark":
        got = gpu.ctx.add_watermark(None, PAY1, both[:n], out=both[n:])
        want = gpu.ctx.add_watermark(None, PAY1, gpu.dev(x))
    else:
        got = gpu.ctx.add_d(both[:n], fm, 0.01, True, out=both[n:])
        want = gpu.ctx.add_d(gpu.dev(x), fm, 0.01, True)
    t.cuda.synchronize()
    assert same_bits(got, want) and same_bits(both[:n], gpu.dev(x))
    a.check()


# ---- K4: sync_fft (fetch_stereo at index 264 of a placed stream), db and the byte-sized `have` output placed -----------------------
SYNC_FFT_CASES = [(pair, h) for i, pair in enumerate(PAIRS) for h in (i, (i + 3) % 8)]


@pytest.mark.parametrize("pair,have_off", SYNC_FFT_CASES, ids=["%s_have%d" % (PAIR_IDS[PAIRS.index(p)], h) for p, h in SYNC_FFT_CASES])
def test_sync_fft(gpu, stream70, pair, have_off):
    t = gpu.torch
    assert sorted({h for _, h in SYNC_FFT_CASES}) == list(range(8))
    w = stream70
    want_list = np.zeros(40, np.int8)
    want_list[[1, 2, 3, 17, 39]] = 1
    first, last = 2 * (264 + 10 * 1024) + 1, 2 * (264 + 30 * 1024)
    for args in ((None, 0, None), (want_list, first, last)):
        tag = args[0] is not None
        want_db, want_have = cached(("sync_fft", tag), lambda: orc.sync_fft(w, 2, 264, 40, *args))
        al_db, al_have = cached(("sync_fft aligned", tag), lambda: gpu.ctx.sync_fft(gpu.dev(w), 264, 40, *args))
        a = gpu.arena(w.nbytes, nbytes(40, 81), 40)
        xin = a.place(w, t.float32, pair[0])
        db = a.place((40, 81), t.float32, pair[1], name="db")
        have = a.place((40,), t.int8, have_off, name="have")
        got_db, got_have = gpu.ctx.sync_fft(xin, 264, 40, *args, out=(db, have))
        t.cuda.synchronize()
        assert have.data_ptr() % 8 == have_off and db.data_ptr() % 16 == pair[1]
        assert same_bits(got_db, al_db) and same_bits(got_have, al_have)
        a.check()
        a.assert_written(db)
        assert not a.untouched(have)
        assert np.array_equal(got_have.cpu().numpy(), want_have) and (not tag or want_have.sum() == 1)
        assert np.abs(got_db.cpu().numpy() - want_db).max() < 2e-4


# ---- K4 / K5 / K4s / K7 / K8 on a placed stream: the results come back to the host, the input is placed --------------------------------
@pytest.mark.parametrize("in_off", IN_OFFSETS)
def test_search_approx(gpu, stream70, in_off):
    oi, oraw, omean = cached(("search_approx",), lambda: orc.search_approx(None, stream70, 2))
    ai, araw, amean = cached(("search_approx aligned",), lambda: gpu.ctx.search_approx(None, gpu.dev(stream70)))
    a = gpu.arena(stream70.nbytes)
    gi, graw, gmean = gpu.ctx.search_approx(None, a.place(stream70, gpu.torch.float32, in_off))
    assert np.array_equal(gi, ai) and np.array_equal(graw, araw) and np.array_equal(gmean, amean)
    a.check()
    assert np.array_equal(gi, oi) and np.abs(graw - oraw).max() < 5e-5 and np.abs(gmean - omean).max() < 1e-5


@pytest.mark.parametrize("in_off", IN_OFFSETS)
def test_sync_search(gpu, stream70, in_off):
    oi, oq, ob = cached(("sync_search",), lambda: orc.sync_search(None, stream70, 2))
    ai, aq, ab = cached(("sync_search aligned",), lambda: gpu.ctx.sync_search(None, gpu.dev(stream70)))
    a = gpu.arena(stream70.nbytes)
    gi, gq, gb = gpu.ctx.sync_search(None, a.place(stream70, gpu.torch.float32, in_off))
    assert np.array_equal(gi, ai) and np.array_equal(gq, aq) and np.array_equal(gb, ab)
    a.check()
    assert gi.tolist() == oi.tolist() and gb.tolist() == ob.tolist() and len(gi) > 0
    assert np.abs(gq - oq).max() < QUALITY_TOL


@pytest.mark.parametrize("in_off", IN_OFFSETS)
def test_block_soft_bits(gpu, golden, stream70, in_off):
    idx = golden["mix_decode70_index"]
    indices = [idx, idx + 8, len(stream70) - 1000]                               # the last one would read past the end
    want = cached(("mix_decode",), lambda: orc.mix_decode(None, stream70, 2, idx + 8))
    al, al_ok = cached(("soft bits aligned",), lambda: gpu.ctx.block_soft_bits(None, gpu.dev(stream70), indices))
    a = gpu.arena(stream70.nbytes)
    got, ok = gpu.ctx.block_soft_bits(None, a.place(stream70, gpu.torch.float32, in_off), indices)
    assert ok.tolist() == [1, 1, 0]                                              # still refused, not read from the NaN guard
    assert np.array_equal(got.view(np.uint32), al.view(np.uint32)) and np.array_equal(ok, al_ok)
    assert not np.isnan(got).any()
    a.check()
    assert np.abs(got[1] - want).max() < 5e-3 and np.abs(want).mean() > 50


@pytest.mark.parametrize("in_off", IN_OFFSETS)
def test_decode_chunk(gpu, stream70, in_off):
    order = lambda p: (p["time"], p["type"], p["block_type"], p["bits"])
    want = cached(("decode_chunk",), lambda: sorted(orc.decode_chunk(None, stream70, 2, True), key=order))
    aligned = cached(("decode_chunk aligned",), lambda: gpu.ctx.decode_chunk(None, gpu.dev(stream70), True))
    a = gpu.arena(stream70.nbytes)
    got = gpu.ctx.decode_chunk(None, a.place(stream70, gpu.torch.float32, in_off), True)
    assert [full(p) for p in got] == [full(p) for p in aligned]
    a.check()
    got = sorted(got, key=order)
    assert [pkey(p) for p in got] == [pkey(p) for p in want] and any(p["bits"] == PAY1 for p in got)
    for g, w in zip(got, want):
        assert abs(g["sync_quality"] - w["sync_quality"]) < QUALITY_TOL and abs(g["decode_error"] - w["decode_error"]) < 1e-5


# ---- get_watermark: the padded copy of a clip (CLIP mode) and the chunk path (BLOCK mode) read the caller's stream ----------------------
def check_get(gpu, x, ch, in_off, tag, pattern_type):
    want = cached(("get", tag, ch), lambda: orc.get(None, x, ch))
    aligned = cached(("get aligned", tag, ch), lambda: gpu.ctx.get_watermark(None, gpu.dev(x)))
    a = gpu.arena(x.nbytes)
    xin = a.place(x, gpu.torch.float32, in_off)
    got = gpu.ctx.get_watermark(None, xin)
    assert xin.data_ptr() % 16 == in_off
    assert [full(p) for p in got] == [full(p) for p in aligned]                  # incl. sync_quality and decode_error
    a.check()
    assert [pkey(p) for p in got] == [pkey(p) for p in want]
    assert max(abs(g["sync_quality"] - w["sync_quality"]) for g, w in zip(got, want)) < QUALITY_TOL
    assert any(p["bits"] == PAY1 and p["type"] == pattern_type for p in got)


@pytest.mark.parametrize("in_off", IN_OFFSETS)
@pytest.mark.parametrize("ch", [1, 2])
def test_get_watermark_clip_mode(gpu, stream70, ch, in_off):
    clip = np.ascontiguousarray(stream70[20 * 44100: 45 * 44100, :ch])         # 25 s
    check_get(gpu, clip, ch, in_off, "clip25", 1)


@pytest.mark.parametrize("ch,in_off", [(1, 4), (2, 4), (2, 8)])
def test_get_watermark_block_mode(gpu, ch, in_off):
    n = 75 * 44100
    x = cached(("stream75", ch), lambda: orc.add(None, noise(43 + ch, n, ch), ch, PAY1).reshape(n, ch))
    check_get(gpu, x, ch, in_off, "stream75", 0)


def test_get_watermark_batch(gpu):
    """6 clips in one arena, two of them misaligned: clip by clip what the aligned batch and the single calls give"""
    t = gpu.torch
    clips = [noise(2300 + i, (22 + i) * 44100 + 13 * i, 2) for i in range(6)]
    marked = [gpu.ctx.add_watermark(None, PAY1 if i % 2 else PAY2, gpu.dev(c)).cpu().numpy() for i, c in enumerate(clips)]
    one_by_one = [gpu.ctx.get_watermark(None, gpu.dev(m)) for m in marked]
    aligned = gpu.ctx.get_watermark_batch(None, [gpu.dev(m) for m in marked])
    a = gpu.arena(*[m.nbytes for m in marked])
    offsets = [0, 4, 0, 0, 12, 0]
    placed = [a.place(m, t.float32, o, name="clip %d" % i) for i, (m, o) in enumerate(zip(marked, offsets))]
    got = gpu.ctx.get_watermark_batch(None, placed)
    assert [[full(p) for p in c] for c in got] == [[full(p) for p in c] for c in aligned] == [[full(p) for p in c] for c in one_by_one]
    a.check()
    for i in (1, 4):
        want = orc.get(None, marked[i], 2)
        assert [pkey(p) for p in got[i]] == [pkey(p) for p in want]
        assert max(abs(g["sync_quality"] - w["sync_quality"]) for g, w in zip(got[i], want)) < QUALITY_TOL
        assert any(p["bits"] == (PAY1 if i % 2 else PAY2) for p in got[i])


def test_add_get_watermark(gpu):
    t = gpu.torch
    n = 60 * 44100 + 333
    x = noise(2400, n, 2)
    want_pcm = gpu.ctx.add_watermark(None, PAY1, gpu.dev(x))
    want = gpu.ctx.get_watermark(None, want_pcm)
    a = gpu.arena(x.nbytes, x.nbytes)
    xin = a.place(x, t.float32, 4)
    out = a.place((n, 2), t.float32, 12)
    got = gpu.ctx.add_get_watermark(None, PAY1, xin, out)
    t.cuda.synchronize()
    assert [full(p) for p in got] == [full(p) for p in want] and any(p["bits"] == PAY1 for p in got)
    assert same_bits(out, want_pcm)
    a.check()
    a.assert_written(out)
    ref = orc.add(None, x, 2, PAY1).reshape(n, 2)
    g = out.cpu().numpy()
    assert rms(g, ref) < RMS_TOL and np.abs(g - ref).max() < 2e-6
    ref_pats = orc.get(None, ref, 2)
    assert [pkey(p) for p in got] == [pkey(p) for p in ref_pats]
    assert max(abs(g["sync_quality"] - w["sync_quality"]) for g, w in zip(got, ref_pats)) < QUALITY_TOL


# ---- K10 / K11 / K12: resamplers -- the phase-per-thread and LDS-staged stereo kernels only for 8-byte aligned input AND output
# ---- (offsets 0 / 8), the generic kernel otherwise (kernels.hh: the same products and sums in the same order) --------------------------
# 48 <-> 44.1 kHz: the phase-per-thread kernels; 22050 Hz: the generic kernel with its LDS-staged stereo form; 33333 Hz: VResampler
RATES = [(48000, 44100), (44100, 48000), (22050, 44100), (33333, 44100)]


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("n", [1, 5, 50001])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate_in,rate_out", RATES)
def test_resample(gpu, rate_in, rate_out, ch, n, pair):
    t = gpu.torch
    x = noise(700 + n % 89 + ch, n, ch)
    want = cached(("resample", rate_in, rate_out, ch, n), lambda: orc.resample(x, ch, rate_in, rate_out).reshape(-1, ch))
    aligned = cached(("resample aligned", rate_in, rate_out, ch, n), lambda: gpu.ctx.resample(gpu.dev(x), rate_in, rate_out))
    m = gpu.ctx.resample_frames(n, rate_in, rate_out)
    assert m == aligned.shape[0] == want.shape[0]
    a = gpu.arena(x.nbytes, nbytes(m, ch))
    xin = a.place(x, t.float32, pair[0])
    out = a.place((m, ch), t.float32, pair[1])
    got = gpu.ctx.resample(xin, rate_in, rate_out, out=out)
    t.cuda.synchronize()
    assert same_bits(got, aligned)
    a.check()
    a.assert_written(out)
    if rate_in == 33333:
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-6
    else:
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("ratio", [1 / 0.9764, 0.8])
def test_resample_ratio(gpu, ratio, pair):
    t = gpu.torch
    n = 50001
    x = noise(int(ratio * 1000), n, 2)
    want = cached(("resample_ratio", ratio), lambda: orc.resample_ratio(x, 2, ratio).reshape(-1, 2))
    aligned = cached(("resample_ratio aligned", ratio), lambda: gpu.ctx.resample_ratio(gpu.dev(x), ratio))
    m = gpu.ctx.resample_ratio_frames(n, 2, ratio)
    assert m == aligned.shape[0] == want.shape[0]
    a = gpu.arena(x.nbytes, nbytes(m, 2))
    xin = a.place(x, t.float32, pair[0])
    out = a.place((m, 2), t.float32, pair[1])
    got = gpu.ctx.resample_ratio(xin, ratio, out=out)
    t.cuda.synchronize()
    assert same_bits(got, aligned)
    a.check()
    a.assert_written(out)
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-6


@pytest.mark.parametrize("in_off", [4, 12])
def test_detect_speed(gpu, in_off):
    """one replayed clip of tests/test_gpu_speed.py (the marked noise replayed at 0.9764) at a misaligned placement"""
    with open(os.path.join(HERE, "golden", "speed_v1.json")) as f:
        g = json.load(f)
    ch = g["channels"]

    def replay():
        marked = orc.add(SPEED_KEY, orc.gen_noise(SPEED_KEY, g["seconds"] * 44100 * ch), ch, g["payload"])
        return orc.resample_ratio(marked, ch, 1 / 0.9764).reshape(-1, ch)
    z = cached(("replayed",), replay)
    aligned = cached(("detect_speed aligned",), lambda: gpu.ctx.detect_speed(SPEED_KEY, gpu.dev(z)))
    a = gpu.arena(z.nbytes)
    got = gpu.ctx.detect_speed(SPEED_KEY, a.place(z, gpu.torch.float32, in_off))
    assert got == aligned
    a.check()
    assert abs(got[0] - g["cases"]["0.9764"]["detect"]) <= SPEED_TOL and abs(got[0] - 0.9764) / 0.9764 < 2e-4


# ---- PCM staging: the s16le fast path (short4 <-> float4) only for bytes at 8 and floats at 16 byte alignment, the generic converters
# ---- otherwise and for every other format; n % 4 == 3: the last float4 / 8-byte group is partial ----------------------------------------
PCM_FORMATS = [("s16le", 16, 0, False), ("s24be", 24, 0, True), ("u8", 8, 1, False), ("f32le", 32, 2, False)]


@pytest.mark.parametrize("byte_off", range(8))
@pytest.mark.parametrize("float_off", [0, 4, 8, 12])
@pytest.mark.parametrize("name,bits,encoding,big", PCM_FORMATS, ids=[f[0] for f in PCM_FORMATS])
def test_pcm_staging(gpu, name, bits, encoding, big, float_off, byte_off):
    t = gpu.torch
    rng = np.random.default_rng(bits * 10 + encoding)
    x = np.concatenate([rng.uniform(-1.2, 1.2, 100002), [0, 1, -1, 0.99999994, -0.5 / 32768, 0.5 / 32768, 32767 / 32768, 1e-9, -1e-9]]).astype(np.float32)
    n = x.size
    assert n % 4 == 3
    width = bits // 8
    want = _np_encode(x, bits, encoding, big, name == "s16le")
    al_enc = cached(("pcm encode aligned", name), lambda: gpu.ctx.pcm_encode(gpu.dev(x), bits, encoding, big, True))
    al_dec = cached(("pcm decode aligned", name), lambda: gpu.ctx.pcm_decode(gpu.dev(want), bits, encoding, big))
    a = gpu.arena(x.nbytes, n * width, n * width, x.nbytes)
    xin = a.place(x, t.float32, float_off, name="encode in")
    raw_out = a.place((n * width,), t.uint8, byte_off, name="encode out")
    raw_in = a.place(want, t.uint8, byte_off, name="decode in")
    back = a.place((n,), t.float32, float_off, name="decode out")
    got = gpu.ctx.pcm_encode(xin, bits, encoding, big, True, out=raw_out)
    dec = gpu.ctx.pcm_decode(raw_in, bits, encoding, big, out=back)
    t.cuda.synchronize()
    assert raw_out.data_ptr() % 8 == byte_off and raw_in.data_ptr() % 8 == byte_off and xin.data_ptr() % 16 == float_off
    assert same_bits(got, al_enc) and same_bits(dec, al_dec)
    a.check()
    a.assert_written(back)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(dec.cpu().numpy().view(np.uint32), _np_decode(want, bits, encoding, big).view(np.uint32))


# ---- the arena itself on the device (tests/test_placement_arena.py is the same on CPU tensors): these tests can fail ------------------
def test_the_arena_finds_planted_damage_on_the_device(gpu):
    t = gpu.torch
    n = 1025
    x = noise(5, n, 2)

    def arena():
        a = gpu.arena(x.nbytes, x.nbytes)
        return a, a.place(x, t.float32, 4, name="in"), a.place((n, 2), t.float32, 12, name="out")
    a, xin, out = arena()
    a.check()
    assert a.untouched(out) and same_bits(xin, gpu.dev(x))
    a.window(out, 2 * n, 1).fill_(0.0)                                            # one value behind the output
    with pytest.raises(AssertionError, match=rf"behind 'out' damaged: first byte at offset {8 * n} "):
        a.check()
    a, xin, out = arena()
    a.window(out, -1, 1).fill_(0.0)                                               # one value in front of it
    with pytest.raises(AssertionError, match=r"in front of 'out' damaged: first byte at offset -4 "):
        a.check()
    a, xin, out = arena()
    a.bytes_at(xin, 8 * n + a.guard_bytes(xin)[1] - 1, 1).fill_(1)                # the last guard byte of the input
    with pytest.raises(AssertionError, match=r"behind 'in' damaged"):
        a.check()
    a, xin, out = arena()
    assert t.isnan(a.window(xin, 0, 2 * n + 1).sum()) and not t.isnan(xin.sum())  # a read one value too far meets a NaN
    out.zero_()
    a.assert_written(out)
    a.check()
