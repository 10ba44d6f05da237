"""Speed detection for batches of clips (awm_detect_speed_batch_d, awm_debug_speed_scan_batch_d; the batch forms of K12 - K15 in
hip/speed.hip) against the one-clip calls on the same clips: every speed, quality, use flag and score with `==`.

The batch runs the passes of the search for sub-groups of clips in lockstep, an entry of a launch being a (clip, centre) pair.  What
can go wrong is at the edges between the entries: a stride, a row count, a table or a pointer taken from another entry of the launch.
So the clips of a batch differ in length (rows per entry), in key (tables per entry) and in alignment, they come in two orders, and the
byte budget is forced so that the sub-groups hold one clip, two clips with a remainder of one, and all clips.

Material as in test_gpu_speed.py: the oracle's noise, marked and replayed at the three speeds of golden/speed_v1.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEY = bytes(range(16))
KEYS = [KEY, bytes(range(1, 17)), bytes([7] * 16)]
AWM_ERR_ARG = -3
SCAN1 = (25.0, 1.0007, 5, 28)               # seconds, step, n_steps, n_center_steps of the first pass (wmspeed.cc:631)
SCAN2 = (50.0, 1.00035, 1, 0)
SCAN3 = (50.0, 1.00005, 40, 0)


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
    g.dev = lambda a, ch=2: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, ch)).cuda()
    yield g
    awm.set_speed_batch(0)
    awm.set_speed_batch_bytes(0)
    awm.set_speed_params()
    ctx.close()


@pytest.fixture(scope="module")
def clips(gpu):
    """nine stereo clips (host arrays [n][2]): the three replayed 30 s clips, cuts of 20 s, 1.2 s and 0.3 s (fewer than 64 rows: one
    partial K13 tile), 0.2 s (takes no part), an empty clip and 3 s of digital silence"""
    with open(os.path.join(HERE, "golden", "speed_v1.json")) as f:
        golden = json.load(f)
    C_ = golden["channels"]
    assert C_ == 2
    y = orc.add(KEY, orc.gen_noise(KEY, golden["seconds"] * 44100 * C_), C_, golden["payload"])
    rep = {s: np.asarray(orc.resample_ratio(y, C_, 1 / float(s)), np.float32).reshape(-1, 2) for s in ("0.9764", "1.01", "1")}
    cut = lambda a, first, seconds: a[first:first + int(seconds * 44100)]
    return [rep["0.9764"], rep["1.01"], rep["1"], cut(rep["0.9764"], 44100, 20), cut(rep["1.01"], 3 * 44100, 1.2), cut(rep["1"], 5000, 0.3),
            cut(rep["1"], 0, 0.2), np.zeros((0, 2), np.float32), np.zeros((3 * 44100, 2), np.float32)]


SILENT, TOO_SHORT = 8, (6, 7)


@pytest.fixture(scope="module")
def dev_clips(gpu, clips):
    return [gpu.dev(c) for c in clips]


@pytest.fixture(scope="module")
def single(gpu, dev_clips):
    """the one-clip call per (clip, key, patient), computed once: (use, best, quality), or the error code where it raises"""
    cache = {}

    def get(i, key=KEY, patient=False):
        k = (i, key, patient)
        if k not in cache:
            try:
                cache[k] = gpu.ctx.detect_speed(key, dev_clips[i], patient)
            except gpu.awm.AwmError as e:
                assert "failed to setup vresampler with ratio=0.000000" in str(e) and "rc=%d" % AWM_ERR_ARG in str(e)
                cache[k] = (AWM_ERR_ARG, 0.0, 0.0)
        return cache[k]
    return get


def budget_for(gpu, n_frames, per_group, patient=False):
    """a byte budget that holds `per_group` clips of the largest kind of the batch (0: the default, which holds all; 1: one byte, for a
    sub-group holds one clip at least)"""
    if per_group < 2:
        return per_group
    return per_group * max(gpu.awm.speed_batch_plan([n], patient=patient, budget_bytes=1 << 50)[1][0] for n in n_frames if n >= 0.25 * 44100)


def expected_launches(groups, order, patient=False):
    """(K12 = K13 = K14, K15) launches of a batch: a sub-group costs one launch per kernel and pass -- three passes, but one where
    digital silence is its only clip (its second pass has nothing to search) -- and one gather and one energy launch"""
    ids = sorted(set(g for g in groups if g >= 0))
    passes = sum(1 if all(order[i] == SILENT for i, g in enumerate(groups) if g == gid) else 3 for gid in ids)
    return passes, 2 * len(ids)


ORDERS = [[0, 1, 2, 3, 4, 5, 6, 7, 8], [7, 4, 8, 2, 5, 0, 6, 3, 1]]


@pytest.mark.parametrize("per_group", [1, 2, 0], ids=["groups_of_1", "room_for_2_long", "all"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("key_per_clip", [False, True], ids=["one_key", "key_per_clip"])
def test_detect_speed_batch_equals_loop(gpu, clips, dev_clips, single, per_group, order, key_per_clip):
    order = ORDERS[order]
    n_frames = [len(clips[i]) for i in order]
    keys = [KEYS[i % 3] for i in order]                # a clip keeps its key in both orders
    budget = budget_for(gpu, n_frames, per_group)
    groups, _ = gpu.awm.speed_batch_plan(n_frames, budget_bytes=budget)
    sizes = [groups.count(g) for g in sorted(set(groups) - {-1})]
    assert [groups[k] for k, i in enumerate(order) if i in TOO_SHORT] == [-1, -1]
    # room for two 30 s clips: two clips, or three short ones (the budget is bytes, not clips) -- or two and a remainder of one
    assert sizes == {1: [1] * 7, 2: [[2, 2, 3], [2, 2, 2, 1]][ORDERS.index(order)], 0: [7]}[per_group]
    gpu.awm.set_speed_batch_bytes(budget)
    before = gpu.awm.speed_batch_launches()
    try:
        got = gpu.ctx.detect_speed_batch(keys if key_per_clip else KEY, [dev_clips[i] for i in order])
    finally:
        gpu.awm.set_speed_batch_bytes(0)
    after = gpu.awm.speed_batch_launches()
    want = [single(i, keys[k] if key_per_clip else KEY) for k, i in enumerate(order)]
    print("batch", got, "\nloop ", want)
    assert got == want
    passes, k15 = expected_launches(groups, order)
    assert tuple(a - b for a, b in zip(after, before)) == (passes, passes, passes, k15)
    # the material is what the test means it to be: the replayed clips are found, the clip at speed 1 needs no correction
    if not key_per_clip:
        by_clip = {i: got[k] for k, i in enumerate(order)}
        assert abs(by_clip[0][0] - 0.9764) < 3e-4 and abs(by_clip[1][0] - 1.01) < 3e-4 and by_clip[2][0] is None and abs(by_clip[2][1] - 1) < 1e-4
        assert by_clip[6] == by_clip[7] == (None, 0.0, 0.0) and by_clip[SILENT] == (AWM_ERR_ARG, 0.0, 0.0)


def test_two_clips_and_a_remainder_of_one(gpu, clips, dev_clips, single):
    """the three 30 s clips under a budget for two of them"""
    order = [1, 2, 0]
    budget = budget_for(gpu, [len(clips[i]) for i in order], 2)
    assert gpu.awm.speed_batch_plan([len(clips[i]) for i in order], budget_bytes=budget)[0] == [0, 0, 1]
    gpu.awm.set_speed_batch_bytes(budget)
    before = gpu.awm.speed_batch_launches()
    try:
        got = gpu.ctx.detect_speed_batch(KEY, [dev_clips[i] for i in order])
    finally:
        gpu.awm.set_speed_batch_bytes(0)
    assert got == [single(i) for i in order]
    assert tuple(a - b for a, b in zip(gpu.awm.speed_batch_launches(), before)) == (6, 6, 6, 4)


@pytest.mark.parametrize("per_group", [2, 0], ids=["groups_of_2_and_1", "all"])
def test_detect_speed_batch_patient(gpu, clips, dev_clips, single, per_group):
    order = [4, 0, 3]                                  # 1.2 s, 30 s, 20 s; a key each
    n_frames = [len(clips[i]) for i in order]
    budget = budget_for(gpu, n_frames, per_group, patient=True)
    groups, _ = gpu.awm.speed_batch_plan(n_frames, patient=True, budget_bytes=budget)
    assert groups == ([0, 0, 1] if per_group else [0, 0, 0])
    gpu.awm.set_speed_batch_bytes(budget)
    before = gpu.awm.speed_batch_launches()
    try:
        got = gpu.ctx.detect_speed_batch(KEYS, [dev_clips[i] for i in order], patient=True)
    finally:
        gpu.awm.set_speed_batch_bytes(0)
    after = gpu.awm.speed_batch_launches()
    want = [single(i, KEYS[k], True) for k, i in enumerate(order)]
    print("batch", got, "\nloop ", want)
    assert got == want
    n = len(set(groups))
    assert tuple(a - b for a, b in zip(after, before)) == (3 * n, 3 * n, 3 * n, 2 * n)


@pytest.mark.parametrize("ch", [1, 3])
def test_mono_and_three_channels(gpu, ch):
    """the <0> form of K12 and the lone last channel of K13, two short clips of different lengths in one launch"""
    rng = np.random.default_rng(40 + ch)
    xs = [rng.uniform(-1, 1, (n, ch)).astype(np.float32) for n in (int(2.1 * 44100) + 1, int(1.3 * 44100))]
    if ch > 1:
        xs[1][:, ch - 1] = 0                           # its last channel digitally silent: -96 dB per band from it
    dev = [gpu.dev(x, ch) for x in xs]
    got = gpu.ctx.detect_speed_batch(KEYS[:2], dev)
    want = [gpu.ctx.detect_speed(k, d) for k, d in zip(KEYS, dev)]
    print("batch", got, "\nloop ", want)
    assert got == want and all(q > 0 for _, _, q in got)


def test_clip_on_a_four_byte_address_between_sentinels(gpu, clips, single):
    """one stereo clip at an address that is 4 but not 8 byte aligned sends the whole launch through the <0> form; every clip lies inside
    one buffer with NaN on both sides -- a read before or behind a clip would reach the scores"""
    t = gpu.torch
    order = [4, 3, 5, 0]
    guard = 64
    offs, at = [], guard
    for k, i in enumerate(order):
        at += (at & 1) ^ (1 if k == 1 else 0)          # clip 1 of the batch at an odd float offset, the others at even ones
        offs.append(at)
        at += clips[i].size + guard
    host = np.full(at + guard, np.nan, np.float32)
    for off, i in zip(offs, order):
        host[off:off + clips[i].size] = clips[i].ravel()
    buf = t.from_numpy(host).cuda()
    views = [buf[off:off + clips[i].size].view(-1, 2) for off, i in zip(offs, order)]
    assert [v.data_ptr() % 8 for v in views] == [0, 4, 0, 0]
    before = gpu.awm.speed_batch_launches()
    got = gpu.ctx.detect_speed_batch(KEY, views)
    assert gpu.awm.speed_batch_launches()[0] - before[0] == 3
    want = [single(i) for i in order]                  # (the one-clip calls on the aligned copies: the <2> form)
    print("batch", got, "\nloop ", want)
    assert got == want
    assert got[1] == gpu.ctx.detect_speed(KEY, views[1])
    assert np.array_equal(buf.cpu().numpy(), host, equal_nan=True)


def scan_loop(gpu, keys, dev, locs, params, speeds):
    before = gpu.awm.speed_batch_launches()
    scans = [gpu.ctx.speed_scan(k, d, loc, *params, s) for k, d, loc, s in zip(keys, dev, locs, speeds)]
    assert gpu.awm.speed_batch_launches() == before    # the one-clip forms
    return scans


def assert_scans_equal(got, want):
    assert len(got) == len(want)
    for (gs, gq), (ws, wq) in zip(got, want):
        assert gs.shape == ws.shape and gs.tolist() == ws.tolist() and gq.tolist() == wq.tolist()
        assert (wq > 0).any()


def test_scan_batch_equals_per_clip_scans(gpu, clips, dev_clips):
    """every score of a pass, not only the winner: K13 and K14 item by item.  Scan 1 on three lengths (171 centres: the launcher folds
    groups of six), a refinement pass with 1, 3 and 5 speeds per clip (9 centres of 3 speeds: one speed per thread), one centre with
    81 relative speeds per clip (folded in the batch, one speed per thread in the one-clip call)"""
    order = [0, 3, 4]
    dev = [dev_clips[i] for i in order]
    before = gpu.awm.speed_batch_launches()
    locs25 = [gpu.ctx.speed_clip_location(k, d, 25.0) for k, d in zip(KEYS, dev)]
    assert len(set(locs25)) == 3
    assert gpu.awm.speed_batch_launches() == before    # the one-clip gather and energy kernels
    got = gpu.ctx.speed_scan_batch(KEYS, dev, locs25, *SCAN1, [[1.0]] * 3)
    assert tuple(a - b for a, b in zip(gpu.awm.speed_batch_launches(), before)) == (1, 1, 1, 0)
    assert_scans_equal(got, scan_loop(gpu, KEYS, dev, locs25, SCAN1, [[1.0]] * 3))
    assert all(len(s) == 57 * 11 for s, _ in got)
    speeds = [[0.9764], [0.97, 0.9764, 1.2], [0.81, 0.99, 1.0, 1.01, 1.24]]
    got = gpu.ctx.speed_scan_batch(KEYS, dev, locs25, *SCAN2, speeds)
    assert_scans_equal(got, scan_loop(gpu, KEYS, dev, locs25, SCAN2, speeds))
    assert [len(s) for s, _ in got] == [3, 9, 15]
    speeds = [[0.9764], [0.9766], [1.0101]]
    got = gpu.ctx.speed_scan_batch(KEY, dev, locs25, *SCAN3, speeds)
    assert_scans_equal(got, scan_loop(gpu, [KEY] * 3, dev, locs25, SCAN3, speeds))
    assert all(len(s) == 81 for s, _ in got)
    # the unfolded <6> form (groups of six as a grid dimension) for the same pass
    gpu.awm.lib.awm_debug_set_speed_compare_fold(0)
    try:
        unfolded = gpu.ctx.speed_scan_batch(KEY, dev, locs25, *SCAN3, speeds)
    finally:
        gpu.awm.lib.awm_debug_set_speed_compare_fold(1)
    assert_scans_equal(unfolded, got)


def test_refusals_leave_the_outputs_untouched(gpu, dev_clips):
    lib, ctx = gpu.awm.lib, gpu.ctx
    d = [dev_clips[4], dev_clips[5]]
    frames = (C.c_size_t * 2)(d[0].shape[0], d[1].shape[0])
    good = (C.c_void_p * 2)(d[0].data_ptr(), d[1].data_ptr())
    null = (C.c_void_p * 2)(d[0].data_ptr(), None)
    before = gpu.awm.speed_batch_launches()
    for ptrs, ch, rate in ((null, 2, 44100), (good, 0, 44100), (good, 2, 0), (good, 2, -44100)):
        speed, quality, use = np.full(2, 7.0), np.full(2, 7.0), np.full(2, 7, np.int32)
        rc = lib.awm_detect_speed_batch_d(ctx._h, KEY, 0, 2, ptrs, frames, ch, rate, 0, speed.ctypes.data_as(C.c_void_p),
                                          quality.ctypes.data_as(C.c_void_p), use.ctypes.data_as(C.c_void_p))
        assert rc == AWM_ERR_ARG
        assert speed.tolist() == [7.0, 7.0] and quality.tolist() == [7.0, 7.0] and use.tolist() == [7, 7]
    assert gpu.awm.speed_batch_launches() == before    # nothing enqueued
    assert lib.awm_detect_speed_batch_d(ctx._h, KEY, 0, 0, None, None, 2, 44100, 0, None, None, None) == 0
    assert gpu.ctx.detect_speed_batch(KEY, []) == []
    # a null pointer is fine where the clip is empty
    zero = (C.c_size_t * 2)(d[0].shape[0], 0)
    speed, quality, use = np.full(2, 7.0), np.full(2, 7.0), np.full(2, 7, np.int32)
    assert lib.awm_detect_speed_batch_d(ctx._h, KEY, 0, 2, null, zero, 2, 44100, 0, speed.ctypes.data_as(C.c_void_p),
                                        quality.ctypes.data_as(C.c_void_p), use.ctypes.data_as(C.c_void_p)) == 0
    assert (speed[1], quality[1], use[1]) == (0.0, 0.0, 0) and quality[0] > 0


# ---- the batches of clips under speed parameters (awm_get_watermark_batch_d and its forms) ----------------------------------------

@pytest.fixture(scope="module")
def get_clips(gpu, clips):
    """host clips of the batch `get`: the three replayed clips, a plain marked clip (20 s at speed 1) and one longer than a block + 2
    frames (60 s: it goes over the lanes with the one-clip search)"""
    return [clips[0], clips[1], clips[2], clips[2][44100:21 * 44100], np.concatenate([clips[0], clips[1]])]


def to_s16(gpu, x):
    raw = gpu.ctx.pcm_encode(x.contiguous().view(-1), 16, 0, False, True)
    return raw.view(gpu.torch.int16).view(x.shape), gpu.ctx.pcm_decode(raw, 16).view(x.shape)


RATES = [44100, 48000, 44100, 48000, 44100]


def batch_forms(gpu, dev):
    """form -> (batch call, list of single calls, the lengths at 44.1 kHz of the clips whose speed the groups search in sub-groups: the
    short ones, whatever their rate or sample format -- the search reads them in the slices of stage 0; the long clip goes over the lanes)"""
    ctx = gpu.ctx
    s16 = [to_s16(gpu, d) for d in dev]
    n44 = [d.shape[0] for d in dev]
    n44_rates = [int(v) for v in gpu.awm.get_batch_rates_plan(n44, RATES)[1]]
    return {
        "batch": (lambda: ctx.get_watermark_batch(KEY, dev), lambda: [ctx.get_watermark(KEY, d) for d in dev], n44[:4]),
        "keys": (lambda: ctx.get_watermark_batch_keys([KEYS[i % 3] for i in range(len(dev))], dev),
                 lambda: [ctx.get_watermark(KEYS[i % 3], d) for i, d in enumerate(dev)], n44[:4]),
        "rates": (lambda: ctx.get_watermark_batch(KEY, dev, sample_rate=RATES),
                  lambda: [ctx.get_watermark(KEY, d, sample_rate=r) for d, r in zip(dev, RATES)], n44_rates[:4]),
        "s16": (lambda: ctx.get_watermark_batch_s16(KEY, [a for a, _ in s16]), lambda: [ctx.get_watermark(KEY, f) for _, f in s16], n44[:4]),
    }


@pytest.mark.parametrize("speed_params", [dict(detect_speed=True), dict(try_speed=0.9764)], ids=["detect_speed", "try_speed"])
@pytest.mark.parametrize("form", ["batch", "keys", "rates", "s16"])
def test_clip_batches_under_speed_parameters(gpu, get_clips, form, speed_params):
    dev = [gpu.dev(c) for c in get_clips]
    batch, singles, searched = batch_forms(gpu, dev)[form]
    plain_before = batch()
    gpu.awm.set_speed_params(**speed_params)
    try:
        want = singles()
        gpu.awm.set_speed_batch(1)                           # the searches of the short clips as a batch
        frames = searched
        for per_group in (1, 2, 0):
            budget = budget_for(gpu, frames, per_group) if frames else 0
            gpu.awm.set_speed_batch_bytes(budget)
            n_groups = len(gpu.awm.speed_batch_plan(frames)[1]) if frames else 0
            before = gpu.awm.speed_batch_launches()
            got = batch()
            delta = tuple(a - b for a, b in zip(gpu.awm.speed_batch_launches(), before))
            assert got == want, (form, per_group)
            # which path ran: a sub-group costs one launch per kernel and pass; --try-speed searches nothing
            k = 3 * n_groups if "detect_speed" in speed_params else 0
            assert delta == (k, k, k, 2 * k // 3), (form, per_group, delta)
        gpu.awm.set_speed_batch_bytes(0)
        for mode in (0, 2):                                  # every clip over the lanes, one-clip searches (the default); one after the other
            gpu.awm.set_speed_batch(mode)
            before = gpu.awm.speed_batch_launches()
            assert batch() == want, mode
            assert gpu.awm.speed_batch_launches() == before
    finally:
        gpu.awm.set_speed_batch(0)
        gpu.awm.set_speed_batch_bytes(0)
        gpu.awm.set_speed_params()
    if form in ("batch", "s16"):
        payload = "0123456789abcdef0011223344556677"
        stretched = [any(p["bits"] == payload and p["speed"] != 1 for p in b) for b in want]
        if "detect_speed" in speed_params:
            assert stretched == [True, True, False, False, True]
            assert all(any(p["bits"] == payload for p in b) for b in want)
        else:
            assert stretched[0] and not stretched[2] and not stretched[3]
    assert batch() == plain_before                           # no state is left behind
