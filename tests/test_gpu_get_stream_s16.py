"""Whole streams straight from signed 16-bit PCM (awm_get_watermark_s16_d, awm_get_watermark_keys_s16_d, awm_get_watermark_rate_s16_d and
the kernel level awm_sync_fft_s16_d, awm_sync_search_s16_d, awm_block_soft_bits_s16_d, awm_debug_sync_db_sliding_rows_s16_d; DESIGN.md
section 10.5).

The definition is exact: with f = pcm_decode of the stream (float (v) * (1 / 32768), no rounding), every 16-bit entry point returns field for
field and bit for bit what its float twin returns for f.  So the reference side of every comparison here is the EXISTING float entry point
on `ctx.pcm_decode` of the same bytes -- never the code under test -- kernel outputs are compared as int32 views, pattern lists as whole
dicts, and there is no tolerance anywhere in this file.

For every marked stream the CPU oracle (_oracle.get, cached per material) first has to find the payload in the decoded 16-bit material, and
the GPU list has to contain it: equality is never between two empty lists.

Shapes: K4's tile is 32 frames (counts 31, 32, 33, 65); K4s flushes every 16 (mono) / 32 (stereo) offsets and fetches blocks of 16
(counts 0, 1, 16, 17, 32, 33, 64, 65); K4b runs 8 blocks per round (1, 8, 9 blocks); ClipDecoder below 3.1 blocks; at least 3 chunks on
several lanes."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc
import _sliding as S
from _placement import CANARY, Arena, need
from test_gpu_get_rate import ERR_ARG, MATERIALS, PAY1, PAY2, cached, gpu, launches, material, with_gaps      # noqa: F401 (gpu: the fixture)
from test_gpu_get_s16 import to_s16

pytestmark = pytest.mark.gpu

FRAME = 1024
BLOCK_FRAMES = 2226                              # 510 sync + 858 x 2 data frames
FLOAT_DB_SCOPES = ("sync_db_kernel(approx)", "sync_db_kernel(refine)", "sync_db_kernel(block)")
S16_DB_SCOPES = ("sync_db_s16_kernel(approx)", "sync_db_s16_kernel(refine)", "sync_db_s16_kernel(block)")
DECODE_SCOPE = "pcm_decode_kernel"
SENTINEL_BITS = 0x7fc0dead
HAVE_SENTINEL = 0x7f
_ORACLE = {}


def with_extremes_and_gap(x):
    """full scale on both sides (32767 and -32768 after the encode) at both ends and in the middle, and a gap of digital silence"""
    x = x.clone()
    n = x.shape[0]
    x[n // 5: n // 5 + 3 * FRAME + 100] = 0
    flat = x.view(-1)
    m = flat.numel()
    for k, v in ((0, 1.0), (1, -1.0), (m - 1, -1.0), (m - 2, 1.0), (m // 2, -1.0), (m // 2 + 1, 1.0)):
        flat[k] = v
    return x


def shifted(gpu, s16, values, pad=4096):
    """a copy of the stream that begins `values` int16 values behind a 16-byte boundary, with alternating full scale in front and behind"""
    t = gpu.torch
    flat = t.empty(s16.numel() + 2 * pad + 8, dtype=t.int16, device="cuda")
    flat[0::2] = 32767
    flat[1::2] = -32768
    assert flat.data_ptr() % 16 == 0 and (2 * pad) % 16 == 0
    flat[pad + values: pad + values + s16.numel()].copy_(s16.reshape(-1))
    out = flat[pad + values: pad + values + s16.numel()].view(s16.shape)
    assert out.data_ptr() % 16 == (2 * values) % 16 and out.is_contiguous()
    return out


def oracle_finds(name, decoded, ch, payload, key=None):
    """the CPU oracle's `get` of the decoded material finds the payload (once per material)"""
    if name not in _ORACLE:
        _ORACLE[name] = orc.get(key, decoded.cpu().numpy(), ch)
    assert any(p["bits"] == payload for p in _ORACLE[name]), (name, "the oracle does not find the payload")


def marked(gpu, name, seed, seconds, ch, payload=PAY1, key=None, rate=44100):
    """(16-bit stream, its decode) of noise marked with the payload, cached"""
    def make():
        n = int(seconds * rate)
        if rate == 44100:
            w = gpu.ctx.add_watermark(key, payload, gpu.noise(seed, n, ch))
        else:
            w = gpu.ctx.add_watermark(key, payload, gpu.noise(seed, n, ch), sample_rate=rate)
        return to_s16(gpu, w)
    return cached(("stream_s16", name), make)


def lane_pcm_bytes(gpu):
    return gpu.lib.awm_debug_lane_pcm_bytes(gpu.ctx._h)


def no_float_path(gpu, counts, what):
    assert counts[DECODE_SCOPE] == 0, (what, counts)
    assert all(counts[s] == 0 for s in FLOAT_DB_SCOPES), (what, counts)
    assert counts["resample_kernel"] == 0 and counts["resample_var_kernel"] == 0, (what, counts)


def get_both(gpu, s16, decoded, payload, what, key=None):
    """get_watermark_s16 against get_watermark on the decode, with the launch and workspace assertions of the default-parameter path"""
    want = gpu.ctx.get_watermark(key, decoded)
    assert gpu.lib.awm_ctx_trim(gpu.ctx._h) == 0
    before = lane_pcm_bytes(gpu)
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_s16(key, s16))
    assert got == want, what
    if payload is not None:
        assert any(p["bits"] == payload for p in got), what
    no_float_path(gpu, counts, what)
    assert lane_pcm_bytes(gpu) == before == 0, what
    return got, counts


# ---- 1. K4: sync_fft_s16 against sync_fft ---------------------------------------------------------------------------------------------
K4_FRAMES = 70 * FRAME + 517


def k4_calls(C):
    """(index, count, first, last, want_frames): frame counts on both sides of the 32-frame tile, an even and an odd index, a last frame
    that ends on the stream's last sample, the borders of the skip rule (tests/test_gpu_frames_edges.py) and a want_frames run"""
    n = K4_FRAMES
    calls = []
    for i, count in enumerate((31, 32, 33, 65)):
        calls.append(((1000, 517)[i % 2], count, 0, None, None))
        calls.append((n - FRAME * count, count, 0, None, None))
    for index in (517, 1000):
        for shift in (0, 1):
            calls.append((index, 40, (index + 4 * FRAME) * C + shift, (index + 36 * FRAME) * C - shift, None))
    want = np.array([1, 0] + [1] * 32 + [0] + [1] * 33, np.int8)
    calls.append((0, len(want), 0, None, want))
    calls.append((333, len(want), (333 + 5 * FRAME) * C + 1, (333 + 60 * FRAME) * C, want))
    return calls


def k4_reference(gpu, C):
    """(16-bit material, per call (dB bits, have) of sync_fft on its decode with sentinel-filled outputs), computed once per channel count"""
    t = gpu.torch

    def make():
        s16, dec = to_s16(gpu, with_extremes_and_gap(gpu.noise(6100 + C, K4_FRAMES, C)))
        assert int(s16.min()) == -32768 and int(s16.max()) == 32767
        refs = []
        for index, count, first, last, want in k4_calls(C):
            db = t.empty((count, 81), dtype=t.float32, device="cuda")
            db.view(t.int32).fill_(CANARY)
            have = t.full((count,), HAVE_SENTINEL, dtype=t.int8, device="cuda")
            gpu.ctx.sync_fft(dec, index, count, want, first, last, out=(db, have))
            refs.append((db.view(t.int32).clone(), have.clone()))
        return s16, refs
    return cached(("k4_ref", C), make)


@pytest.mark.parametrize("offset", (0, 2, 4, 6, 14))
@pytest.mark.parametrize("C", (2, 1, 3), ids=("stereo", "mono", "three"))
def test_k4_sync_fft(gpu, C, offset):
    """the stream in an Arena at the byte offset (stereo at offset 2: frames that are only 2-byte aligned), between runs of alternating
    full scale; outputs in the Arena too, between canaries"""
    t = gpu.torch
    s16, refs = k4_reference(gpu, C)
    calls = k4_calls(C)
    pad = 2048                                                            # values of +-full scale on either side (4096 bytes: the offset survives)
    host = np.empty(2 * pad + s16.numel(), np.int16)
    host[0::2], host[1::2] = 32767, -32768
    host[pad: pad + s16.numel()] = s16.cpu().numpy().reshape(-1)
    arena = Arena(t, need(host.nbytes, *[c[1] * 81 * 4 for c in calls], *[c[1] for c in calls]), device="cuda")
    placed = arena.place(host, t.int16, offset)
    stream = placed[pad: pad + s16.numel()].view(s16.shape)
    assert stream.data_ptr() % 16 == offset and stream.is_contiguous()
    seen_skip = False
    for (index, count, first, last, want), (ref_db, ref_have) in zip(calls, refs):
        db = arena.place((count, 81), t.float32, 0)
        have = arena.place((count,), t.int8, 0)
        have.fill_(HAVE_SENTINEL)
        gpu.ctx.sync_fft_s16(stream, index, count, want, first, last, out=(db, have))
        what = (C, offset, index, count, first, last, want is not None)
        assert t.equal(db.view(t.int32), ref_db), what
        assert t.equal(have, ref_have), what
        seen_skip |= bool((ref_have == 0).any()) and bool((ref_have == 1).any())
    assert seen_skip
    gpu.ctx.synchronize()
    arena.check()


# ---- 2. K4s in the product layout -----------------------------------------------------------------------------------------------------
K4S_FRAMES = 16384
GAP0, GAP_LEN = 5000, FRAME + 8 * 20            # a window that starts at GAP0 is empty, and stays so for 20 offsets
LONE_GAP0, LONE_AT = 9000, 9000 + 700           # a second gap with one non-zero sample inside


def k4s_streams():
    """(bases, counts): the counts 0, 1, 16, 17, 32, 33, 64, 65; odd and even bases; windows ending on the last sample; a window that runs
    empty exactly at a block-of-16 border (offset 16); a lone non-zero sample at window position 0"""
    n = K4S_FRAMES
    bases = [100, 517, GAP0 - 8 * 16, LONE_AT, 2000, 3001, n - FRAME - 8 * 15, n - FRAME - 8 * 64]
    counts = [0, 1, 64, 17, 32, 33, 16, 65]
    return np.array(bases, np.int64), np.array(counts, np.int32)


def k4s_material(gpu, C):
    def make():
        x = gpu.noise(6200 + C, K4S_FRAMES, C).clone()
        x[GAP0: GAP0 + GAP_LEN] = 0
        x[LONE_GAP0: LONE_GAP0 + 3 * FRAME] = 0
        x[LONE_AT] = 0.5
        x.view(-1)[0], x.view(-1)[-1] = 1.0, -1.0
        return to_s16(gpu, x)
    return cached(("k4s", C), make)


def k4s_launch(gpu, call, pcm, C, bases, counts, perm, pos):
    t = gpu.torch
    rpp, n_slots = 4, 12                                                   # two planes of streams, a third that stays untouched
    ld, with_tail = (64, True) if C == 2 else (72, False)
    out = t.empty((n_slots, S.ROWS, ld), dtype=t.float32, device="cuda")
    out.view(t.int32).fill_(SENTINEL_BITS)
    tail = None
    if with_tail:
        tail = t.empty((n_slots, S.ROWS + 4), dtype=t.float32, device="cuda")
        tail.view(t.int32).fill_(SENTINEL_BITS)
    have = t.full((n_slots, 72), HAVE_SENTINEL, dtype=t.int8, device="cuda")
    call(pcm, K4S_FRAMES, bases, counts, 65, rpp, perm, pos, 0, K4S_FRAMES * C, out, have, tail=tail)
    return out.view(t.int32), (tail.view(t.int32) if with_tail else None), have


@pytest.mark.parametrize("C", (2, 1), ids=("stereo", "mono"))
def test_k4s_sliding_rows(gpu, C):
    """stereo: ld = 64 + tail (sync_db_sliding4_kernel's layout); mono: ld = 72"""
    t = gpu.torch
    s16, dec = k4s_material(gpu, C)
    dev = lambda a: t.from_numpy(np.ascontiguousarray(a)).cuda()
    bases, counts = k4s_streams()
    perm, pos = S.random_tables(np.random.default_rng(62), 1, 4)
    tabs = (dev(bases), dev(counts), dev(perm), dev(pos))
    want = k4s_launch(gpu, gpu.ctx.sync_db_sliding_rows, dec, C, *tabs)
    assert bool((want[0] != SENTINEL_BITS).any()) and bool((want[2] == 1).any()) and bool((want[2] == HAVE_SENTINEL).any())
    if C == 2:
        assert bool((want[1][:, :S.ROWS] != SENTINEL_BITS).any())              # the stream of 65 offsets wrote its tail
    # -96 dB per channel where the window is empty: the gap stream from offset 16 on, the lone sample's stream at offset 0
    silent = np.float32(-96.0 * C).view(np.int32)
    assert bool((want[0] == int(silent)).any())
    for values in (0, 2, 1, 3):                                             # the base at 4-byte addresses, then at 2-byte-only ones
        stream = shifted(gpu, s16, values)
        assert stream.data_ptr() % 4 == 2 * (values % 2)
        got = k4s_launch(gpu, gpu.ctx.sync_db_sliding_rows_s16, stream, C, *tabs)
        for g, w, what in zip(got, want, ("rows", "tail", "have")):
            assert (g is None and w is None) or t.equal(g, w), (C, values, what)


# ---- 3. K4b + K7: block_soft_bits_s16 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (2, 1, 3), ids=("stereo", "mono", "three"))
def test_k4b_block_soft_bits(gpu, C):
    n = BLOCK_FRAMES * FRAME + 9000
    s16, dec = cached(("k4b", C), lambda: to_s16(gpu, with_extremes_and_gap(gpu.noise(6300 + C, n, C))))
    end = n - BLOCK_FRAMES * FRAME
    index = [0, 517, end, end + 1, 1000, 2001, 3002, 4003, 5004]            # block 2 ends on the last sample, block 3 reads past it
    for nb in (1, 8, 9):
        want, want_ok = gpu.ctx.block_soft_bits(None, dec, index[:nb])
        for values in (0, 1):
            got, got_ok = gpu.ctx.block_soft_bits_s16(None, shifted(gpu, s16, values), index[:nb])
            assert np.array_equal(got_ok, want_ok), (C, nb, values)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (C, nb, values)
        if nb >= 4:
            assert list(want_ok[:4]) == [1, 1, 1, 0]
        assert np.abs(want[:nb][want_ok[:nb] == 1]).max() > 0


# ---- 4. sync_search_s16 --------------------------------------------------------------------------------------------------------------
def search_equal(gpu, s16, dec, clip_mode, what):
    want = gpu.ctx.sync_search(None, dec, clip_mode)
    got, counts = launches(gpu, lambda: gpu.ctx.sync_search_s16(None, s16, clip_mode))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), what
    no_float_path(gpu, counts, what)
    return want, counts


def test_sync_search_block_mode(gpu):
    s16, dec = marked(gpu, "stereo75", 6400, 75, 2)
    oracle_finds("stereo75", dec, 2, PAY1)
    want, counts = search_equal(gpu, s16, dec, False, "block mode")
    assert len(want[0]) > 0
    assert counts["sync_db_s16_kernel(approx)"] == 1 and counts["sync_db_s16_kernel(refine)"] >= 1, counts


@pytest.mark.parametrize("kind", MATERIALS)
def test_sync_search_clip_mode(gpu, kind):
    """25 s clips; all-zero, only the first and only the last value non-zero put the silence scan on int16"""
    s16, dec = to_s16(gpu, material(gpu, kind, 6410, 25 * 44100, 2))
    if kind == "first":
        assert int(s16.view(-1)[0]) != 0 and not bool(s16.view(-1)[1:].any())
    if kind == "last":
        assert int(s16.view(-1)[-1]) != 0 and not bool(s16.view(-1)[:-1].any())
    search_equal(gpu, s16, dec, True, kind)
    search_equal(gpu, shifted(gpu, s16, 1), dec, True, kind + " at a 2-byte address")


# ---- 5. get_watermark_s16 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", (2, 1), ids=("stereo", "mono"))
def test_get_marked_stream(gpu, ch):
    name = "stereo75" if ch == 2 else "mono75"
    s16, dec = marked(gpu, name, 6400 if ch == 2 else 6401, 75, ch)
    oracle_finds(name, dec, ch, PAY1)
    _, counts = get_both(gpu, s16, dec, PAY1, name)
    assert all(counts[s] > 0 for s in S16_DB_SCOPES), counts
    # 75 s: the block decoder's search and the ClipDecoder's START and END searches, on 16-bit padded copies
    assert counts["sync_db_s16_kernel(approx)"] == 3, counts
    # ... and at an address that is only 2-byte aligned
    assert gpu.ctx.get_watermark_s16(None, shifted(gpu, s16, 1)) == gpu.ctx.get_watermark(None, dec)


def test_get_clip_of_25_s(gpu):
    s16, dec = marked(gpu, "clip25", 6402, 25, 2, PAY2)
    oracle_finds("clip25", dec, 2, PAY2)
    _, counts = get_both(gpu, s16, dec, PAY2, "clip25")
    # no room for a block and not more than one long block: the ClipDecoder's START search alone
    assert counts["sync_db_s16_kernel(approx)"] == 1 and counts["sync_db_s16_kernel(block)"] > 0, counts


def test_get_around_3_1_blocks(gpu):
    """the ClipDecoder runs below 3.1 blocks of frames and not from there on"""
    border = int(BLOCK_FRAMES * 3.1 * FRAME)
    s16, dec = marked(gpu, "blocks3_1", 6403, (border + 3 * FRAME) / 44100 + 0.01, 2)
    assert s16.shape[0] >= border + 2 * FRAME
    under, over = border - FRAME, border + FRAME
    oracle_finds("blocks3_1", dec[:under], 2, PAY1)
    _, c_under = get_both(gpu, s16[:under], dec[:under], PAY1, "just under 3.1 blocks")
    _, c_over = get_both(gpu, s16[:over], dec[:over], PAY1, "just over 3.1 blocks")
    assert c_under["sync_db_s16_kernel(approx)"] == 3 and c_over["sync_db_s16_kernel(approx)"] == 1, (c_under, c_over)


def test_get_empty_and_shorter_than_a_frame(gpu):
    t = gpu.torch
    for n in (0, 1, FRAME - 1):
        for ch in (1, 2):
            x16 = t.full((n, ch) if ch > 1 else (n,), 1234, dtype=t.int16, device="cuda")
            dec = gpu.ctx.pcm_decode(x16.view(t.uint8).view(-1), 16).view(x16.shape) if n else t.zeros(x16.shape, dtype=t.float32, device="cuda")
            assert gpu.ctx.get_watermark_s16(None, x16) == gpu.ctx.get_watermark(None, dec), (n, ch)


@pytest.mark.parametrize("fpb", (1, 3))
def test_get_frames_per_bit(gpu, fpb):
    gpu.awm.set_params(frames_per_bit=fpb)
    orc.set_params(frames_per_bit=fpb)
    try:
        name = "fpb%d" % fpb
        s16, dec = marked(gpu, name, 6404 + fpb, 45 if fpb == 1 else 80, 2)
        oracle_finds(name, dec, 2, PAY1)
        _, counts = get_both(gpu, s16, dec, PAY1, name)
        assert all(counts[s] > 0 for s in S16_DB_SCOPES), counts
    finally:
        gpu.awm.set_params()
        orc.set_params()


def test_get_two_keys(gpu):
    keys = [gpu.awm.test_key(1), gpu.awm.test_key(2)]
    s16, dec = marked(gpu, "key2", 6408, 75, 2, PAY2, key=keys[1])
    oracle_finds("key2", dec, 2, PAY2, key=keys[1])
    want = gpu.ctx.get_watermark_keys(keys, dec)
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_keys_s16(keys, s16))
    assert got == want                                                      # whole dicts: key_index included
    assert any(p["bits"] == PAY2 and p["key_index"] == 1 for p in got)
    no_float_path(gpu, counts, "two keys")
    # the dB planes of an approximate search are shared by the keys: the block decoder's, the ClipDecoder's START and END
    assert counts["sync_db_s16_kernel(approx)"] == 3, counts


def test_get_several_chunks_on_several_lanes(gpu):
    """about 8 min with get_chunk_size just above the chunk overlap (2 x 1.3 blocks = 2.24 min): the chunks are views of the int16 stream"""
    s16, dec = marked(gpu, "min8", 6409, 8 * 60, 2)
    oracle_finds("min8", dec, 2, PAY1)
    gpu.awm.set_params(chunk_size_min=3.0)
    try:
        chunks = gpu.awm.plan_chunks(s16.shape[0])
        assert len(chunks) >= 3
        _, counts = get_both(gpu, s16, dec, PAY1, "8 min in chunks")
        assert counts["sync_db_s16_kernel(approx)"] == len(chunks), (counts, len(chunks))
    finally:
        gpu.awm.set_params()


# ---- 6. rates -------------------------------------------------------------------------------------------------------------------------
def test_rate_48000_phase_form(gpu):
    s16, dec = marked(gpu, "r48", 6500, 75, 2, PAY2, rate=48000)
    if "r48" not in _ORACLE:
        _ORACLE["r48"] = orc.get(None, orc.resample(dec.cpu().numpy(), 2, 48000, 44100), 2)
    assert any(p["bits"] == PAY2 for p in _ORACLE["r48"])
    want = gpu.ctx.get_watermark(None, dec, sample_rate=48000)
    assert gpu.lib.awm_ctx_trim(gpu.ctx._h) == 0
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_s16(None, s16, sample_rate=48000))
    assert got == want and any(p["bits"] == PAY2 for p in got)
    # the resampler reads the 16-bit values; behind it the call is the float call's, on the lane's 44.1 kHz copy
    assert counts[DECODE_SCOPE] == 0 and counts["resample_kernel"] == 0 and counts["resample_var_kernel"] == 0, counts
    assert counts["resample_s16_kernel"] == 1 and lane_pcm_bytes(gpu) == 0, counts
    # frames that are only 2-byte aligned: the generic taps, the same bits
    assert gpu.ctx.get_watermark_s16(None, shifted(gpu, s16, 1), sample_rate=48000) == want


def test_rate_32000_generic_form(gpu):
    s16, dec = marked(gpu, "r32", 6501, 75, 2, PAY1, rate=32000)
    want = gpu.ctx.get_watermark(None, dec, sample_rate=32000)
    assert any(p["bits"] == PAY1 for p in want)
    assert gpu.lib.awm_ctx_trim(gpu.ctx._h) == 0
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_s16(None, s16, sample_rate=32000))
    assert got == want
    assert counts[DECODE_SCOPE] == 0 and counts["resample_kernel"] == 0 and counts["resample_var_kernel"] == 0, counts
    assert counts["resample_s16_kernel"] == 1 and lane_pcm_bytes(gpu) == 0, counts


def test_rate_44101_vresampler_decodes_on_the_lane(gpu):
    """the documented exception: a rate that only the VResampler takes is decoded into the lane's workspace first"""
    s16, dec = marked(gpu, "stereo75", 6400, 75, 2)
    want = gpu.ctx.get_watermark(None, dec, sample_rate=44101)
    assert any(p["bits"] == PAY1 for p in want)
    got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_s16(None, s16, sample_rate=44101))
    assert got == want
    assert counts[DECODE_SCOPE] == 1 and counts["resample_var_kernel"] >= 1 and counts["resample_s16_kernel"] == 0, counts
    assert all(counts[s] == 0 for s in S16_DB_SCOPES), counts               # behind the resampler the call is the float call
    assert lane_pcm_bytes(gpu) >= s16.numel() * 4
    assert gpu.lib.awm_ctx_trim(gpu.ctx._h) == 0 and lane_pcm_bytes(gpu) == 0


# ---- 7. speed parameters --------------------------------------------------------------------------------------------------------------
def speed_material(gpu):
    def make():
        w = gpu.ctx.add_watermark(None, PAY1, gpu.noise(6600, int(75 * 1.02 * 44100) + 2000, 2))
        return to_s16(gpu, gpu.ctx.resample_ratio(w, 1 / 1.02).contiguous())
    return cached(("stream_s16", "speed102"), make)


@pytest.mark.parametrize("mode", ("try_speed", "detect_speed"))
def test_speed_parameters(gpu, mode):
    """the lane decodes the chunk for the speed part (documented); the lists are the float call's"""
    s16, dec = speed_material(gpu)
    orc.set_speed_params(False, False, 1.02)
    try:
        oracle_finds("speed102", dec, 2, PAY1)
    finally:
        orc.set_speed_params(False, False, -1)
    if mode == "try_speed":
        gpu.awm.set_speed_params(try_speed=1.02)
    else:
        gpu.awm.set_speed_params(detect_speed=True)
    try:
        want = gpu.ctx.get_watermark(None, dec)
        got, counts = launches(gpu, lambda: gpu.ctx.get_watermark_s16(None, s16))
        assert got == want
        assert any(p["bits"] == PAY1 for p in got)
        assert counts[DECODE_SCOPE] == 1, counts                            # one chunk, decoded once on its lane
        assert counts["sync_db_s16_kernel(approx)"] >= 1, counts            # the un-stretched decoders read the 16-bit values
    finally:
        gpu.awm.set_speed_params()
        gpu.lib.awm_ctx_trim(gpu.ctx._h)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    t, lib, h = gpu.torch, gpu.lib, gpu.ctx._h
    s16, _ = marked(gpu, "clip25", 6402, 25, 2, PAY2)
    n = s16.shape[0]
    key = gpu.awm.key_bytes(None)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    dev = lambda a: C.c_void_p(a.data_ptr())
    db = t.empty((4, 81), dtype=t.float32, device="cuda")
    have = t.empty((4,), dtype=t.int8, device="cuda")
    rows = t.empty((4, S.ROWS, 64), dtype=t.float32, device="cuda")
    tail = t.empty((4, S.ROWS), dtype=t.float32, device="cuda")
    rhave = t.empty((4, 72), dtype=t.int8, device="cuda")
    bases = t.zeros(4, dtype=t.int64, device="cuda")
    cnts = t.ones(4, dtype=t.int32, device="cuda")
    perm, pos = S.random_tables(np.random.default_rng(8), 1, 4)
    perm, pos = t.from_numpy(perm).cuda(), t.from_numpy(pos).cuda()

    def attempt(ptr, frames, what):
        pats = np.full(8 * 256, 0x5a, np.uint8)
        which = np.full(8, -7, np.int32)
        idx, q, bt = np.full(8, 77, np.uint64), np.full(8, -7.0), np.full(8, -7, np.int32)
        soft, ok, blocks = np.full(858, -7.0, np.float32), np.full(1, -7, np.int32), np.zeros(1, np.uint64)
        for buf in (db, rows, tail):
            buf.view(t.int32).fill_(CANARY)
        have.fill_(HAVE_SENTINEL)
        rhave.fill_(HAVE_SENTINEL)
        calls = (lambda: lib.awm_get_watermark_s16_d(h, key, ptr, frames, 2, 8, vp(pats)),
                 lambda: lib.awm_get_watermark_keys_s16_d(h, key + key, 2, ptr, frames, 2, 8, vp(pats), vp(which)),
                 lambda: lib.awm_get_watermark_rate_s16_d(h, key, ptr, frames, 2, 48000, 8, vp(pats)),
                 lambda: lib.awm_get_watermark_rate_s16_d(h, key, ptr, frames, 2, 44100, 8, vp(pats)),
                 lambda: lib.awm_sync_fft_s16_d(h, ptr, frames, 2, 0, 4, None, 0, 2 * frames, dev(db), dev(have)),
                 lambda: lib.awm_sync_search_s16_d(h, key, ptr, frames, 2, 1, 8, vp(idx), vp(q), vp(bt)),
                 lambda: lib.awm_block_soft_bits_s16_d(h, key, ptr, frames, 2, vp(blocks), 1, vp(soft), vp(ok)),
                 lambda: lib.awm_debug_sync_db_sliding_rows_s16_d(h, ptr, frames, 2, dev(bases), dev(cnts), 4, 1, 4, dev(perm), dev(pos), 0, 2 * frames,
                                                                  None, None, 1, 0, 64, dev(rows), dev(tail), S.ROWS, dev(rhave), 72))

        def run():
            return [call() for call in calls]
        rcs, counts = launches(gpu, run)
        assert rcs == [ERR_ARG] * len(calls), (what, rcs)
        assert sum(counts.values()) == 0, (what, counts)
        assert (pats == 0x5a).all() and (which == -7).all() and (idx == 77).all() and (q == -7).all() and (bt == -7).all(), what
        assert (soft == -7).all() and (ok == -7).all(), what
        for buf in (db, rows, tail):
            assert bool((buf.view(t.int32) == CANARY).all()), what
        assert bool((have == HAVE_SENTINEL).all()) and bool((rhave == HAVE_SENTINEL).all()), what

    attempt(C.c_void_p(s16.data_ptr() + 1), n - 1, "an odd pointer")
    attempt(None, n, "NULL with frames")
    for form in (0, 3, 5):
        lib.awm_debug_set_refine_form(form)
        try:
            attempt(C.c_void_p(s16.data_ptr()), n, "refine form %d" % form)
        finally:
            lib.awm_debug_set_refine_form(4)
    # ... and with the default form back, the same pointers are taken
    assert lib.awm_sync_fft_s16_d(h, C.c_void_p(s16.data_ptr()), n, 2, 0, 4, None, 0, 2 * n, dev(db), dev(have)) == 0
    gpu.ctx.synchronize()
    assert not bool((db.view(t.int32) == CANARY).any())
