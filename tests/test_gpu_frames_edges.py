"""K4 and K4b (csrc/hip/kernels.hip sync_db_kernel) held to a float64 transform value by value, and K7 (soft_bits_wave_kernel /
soft_bits_kernel) held bit for bit to its restatement evaluated on K7's own inputs.

The yardsticks are tests/_frames.py: ref_db_frames / channel_frames (float64 rfft, analytic von Hann window, the reference's last float
steps) with a tolerance derived per value -- the sensitivity to delta = K_FFT eps32 ||x w||_2 in re and im + 4 ulp32, K_FFT measured on
the CPU and never against the kernels --, and soft_bits / cells_read (the reference's mix_decode restated, with the device's rule for
blocks of padded slices); test_frames_restated.py ties both to the oracle on the CPU.  -96 C, the +0 of skipped or unwanted frames, the
have flags and every sentinel are exact.

    K4   through awm_sync_fft_d: frame counts on both sides of the 32-frame tile, even and odd index, index 0, a last frame that ends
         on the last sample, 1 / 2 / 3 channels (the <1, ...> channel loop and the <2, false, 33> pair transform), first / last ON
         the borders of the skip rule and one value further, want_frames in runs of 1, 32 and 33; every material
    K4b  through awm_debug_block_db_d (the launch of block_soft_bits_dev, the dB workspace prefilled with a quiet NaN): every cell
         of three whole blocks written and within its channel's own tolerance -- stereo the SPLIT kernel (140 tiles of 16 frames, the
         last one of 2), mono and three channels the blockIdx.z planes; a start one sample too late is refused (slot -1)
    K4b + K7 on blocks of padded slices: the first and the last live frame at every residue of 16, live ranges that cover the block's
         frame 0 / its last frame (the reflected neighbours), a single live frame, blocks wholly in the padding, a slice of nothing
         but silence; odd ranges for stereo; three channels at frames_per_bit 3 and the debug switch, where K7 is the kernel that
         loads every cell and K4b therefore writes every cell.  Every cell K7 reads is written, what is left as sentinel is outside cells_read,
         frames outside the live range are exactly -96, live frames within tolerance, and the soft bits equal soft_bits on the
         device's own planes BIT FOR BIT with the sentinels left in place (a stray read shows as NaN) and lie within the summed
         tolerances (weights 1 and 1/2) of soft_bits on the reference planes
    K7   alone through awm_debug_soft_bits_planes_d on hand-made planes of wildly different magnitudes: 1, 7, 8 and 9 blocks (the
         eight-per-round XCD mapping and its tail), stereo and mono, frames_per_bit 2 and 3, with and without live ranges (NaN in every
         cell cells_read leaves out); bit for bit against the restatement, and the one-thread-per-bit kernel
         (awm_debug_set_soft_bits_generic) bit for bit against the wave kernel
A key per block (SoftBitsArgs::block_slice) is not driven: the debug views take one key, the group tables have no entry point.

Each test prints the kernels' largest |got - ref| / tol.  Measured on an MI355X on 2026-10-20, for information (the tolerance is not
tuned to it): K4 white 0.16, sloped 0.30, gaps 0.22, levels 0.51, tone 0.54, pair 0.29; K4b whole blocks 0.70 (stereo and three channels),
0.48 mono; padded slices 0.20."""
import numpy as np
import pytest

import _frames as F
import _oracle as orc

pytestmark = pytest.mark.gpu

SENTINEL_BITS = 0x7fc0dead
NF = F.BLOCK_FRAMES
COUNTS = (1, 2, 31, 32, 33, 63, 64, 65)
SLACK = 18                                      # frames a block may start into its slice
TINY_BLOCK = 6                                  # of K7's hand-made blocks
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    ctx = awm.Context(0)
    yield awm, ctx, torch
    awm.lib.awm_debug_set_soft_bits_generic(0)
    awm.set_params()
    orc.set_params()
    ctx.close()
    _cache.clear()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ratio(got, want, tol, what):
    """every value within its tolerance, to the bit where that is 0 (+0, not -0); returns the largest |got - want| / tol"""
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - want)
        bad = ~(d <= tol)                                            # (a NaN -- an unwritten cell -- is bad)
    bad |= (tol == 0) & (got.view(np.uint32) != want.view(np.uint32))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        worst = np.nanmax(np.where(bad & (tol > 0), d / np.where(tol > 0, tol, 1), 0))
        raise AssertionError("%s: %d of %d values off, worst %.3g x its tolerance, first %s got %r want %r tol %.3g"
                             % (what, int(bad.sum()), got.size, worst, list(map(int, i)), got[i], want[i], tol[i]))
    return float(np.max(np.where(tol > 0, d / np.where(tol > 0, tol, 1), 0), initial=0.0))


# ---- K4 ------------------------------------------------------------------------------------------------------------------------------
MATERIALS = list(F.materials())


def k4_calls(name, C):
    """(index, count, first, last, want_frames) of every launch of a material"""
    n = F.N_FRAMES
    calls = []
    for i, count in enumerate(COUNTS):
        calls.append(((0, 517, 1000)[i % 3], count, 0, None, None))
        calls.append((n - F.FRAME * count, count, 0, None, None))              # the last frame ends exactly on the last sample
    # the skip rule: frame 3 ends exactly at `first`, frame 36 starts exactly at `last` (transformed); one value further they are skipped
    for index in (517, 1000):
        for shift in (0, 1):
            calls.append((index, 40, (index + 4 * F.FRAME) * C + shift, (index + 36 * F.FRAME) * C - shift, None))
    want = np.array([1, 0] + [1] * 32 + [0] + [1] * 33, np.int8)             # runs of 1, 32 and 33, single unwanted frames between
    calls.append((0, len(want), 0, None, want))
    calls.append((333, len(want), (333 + 5 * F.FRAME) * C + 1, (333 + 60 * F.FRAME) * C, want))
    if name == "gaps":
        calls.append((F.LONE_AT % F.FRAME, 65, 0, None, None))                 # the lone sample at window position 0 of frame 31
        calls.append((F.GAP_BOTH[0] - 3 * F.FRAME - 100, 33, 0, None, None))
    return calls


@pytest.mark.parametrize("C", (2, 1, 3), ids=("stereo", "mono", "three"))
@pytest.mark.parametrize("name", MATERIALS)
def test_frames_edges_k4(gpu, name, C):
    awm, ctx, torch = gpu
    x = np.ascontiguousarray(cached("materials", F.materials)[name][:, :C])
    xd = dev(torch, x)
    worst, n_exact = 0.0, 0
    for index, count, first, last, want in k4_calls(name, C):
        got_db, got_have = ctx.sync_fft(xd, index, count, want, first, last)
        got_db, got_have = got_db.cpu().numpy(), got_have.cpu().numpy()
        db, have, tol = F.ref_db_frames(x, index, count, first, last)
        if want is not None:
            db[want == 0], tol[want == 0], have[want == 0] = 0, 0, 0           # unwanted columns keep +0 and have 0
        what = "%s C=%d index %d count %d first %s last %s%s" % (name, C, index, count, first, last, " want" if want is not None else "")
        assert np.array_equal(got_have, have), what
        worst = max(worst, ratio(got_db, db, tol, what))
        n_exact += int((tol == 0).sum())
        if first:
            assert (have == 0).any() and have.any()
    print("K4 %s C=%d: largest |got - ref| / tol = %.3f, %d values exact by rule" % (name, C, worst, n_exact))
    assert n_exact > 0


# ---- K4b, whole blocks ---------------------------------------------------------------------------------------------------------------
def block_reference(x, start, lo=0, hi=NF - 1, nf=NF):
    """(planes [C][81][nf] float32, tol alike): -96 and 0 outside the frames lo .. hi, the transform's values inside"""
    C = x.shape[1]
    planes = np.full((C, F.NB, nf), -96, np.float32)
    tol = np.zeros((C, F.NB, nf))
    if hi >= lo:
        db, sens, fired = F.channel_frames(x, start + lo * F.FRAME, hi - lo + 1)
        planes[:, :, lo:hi + 1] = db.transpose(0, 2, 1)
        tol[:, :, lo:hi + 1] = F.channel_tol(db, sens, fired).transpose(0, 2, 1)
    return planes, tol


@pytest.mark.parametrize("C", (2, 1, 3), ids=("stereo", "mono", "three"))
def test_frames_edges_k4b_whole_blocks(gpu, C):
    awm, ctx, torch = gpu
    x = np.ascontiguousarray(cached("block_pcm", F.block_pcm)[:, :C])
    mix = F.mix_entries(None)
    end = len(x) - NF * F.FRAME
    assert end % 2 == 1
    starts = [0, 777, end, end + 1]                                 # an even and an odd start, the last frame on the last sample, one too far
    planes, soft, slot = ctx.debug_block_db(None, dev(torch, x), starts, fill=SENTINEL_BITS)
    assert slot.tolist() == [0, 1, 2, -1]
    planes = planes.cpu().numpy()
    assert planes.shape == (4, C, F.NB, ctx.block_plane_ld()) and planes.shape[3] >= NF
    bits = planes.view(np.uint32)
    assert (bits[:3, :, :, NF:] == SENTINEL_BITS).all()
    assert not (bits[:3, :, :, :NF] == SENTINEL_BITS).any(), "a cell of a whole block is left unwritten"
    worst = 0.0
    for i, start in enumerate(starts[:3]):
        want, tol = block_reference(x, start)
        worst = max(worst, ratio(np.ascontiguousarray(planes[i, :, :, :NF]), want, tol, "block at %d" % start))
        own = F.soft_bits(planes[i], mix, 2, NF)
        assert np.array_equal(soft[i].view(np.uint32), own.view(np.uint32)), "K7 against its restatement on the device's planes, block at %d" % start
        ref = F.soft_bits(want, mix, 2, NF)
        sum_tol = F.soft_bits_tol(tol, mix, 2, NF)
        assert (np.abs(soft[i].astype(np.float64) - ref) <= sum_tol).all(), float(np.max(np.abs(soft[i] - ref) / sum_tol))
    print("K4b whole blocks C=%d: largest |got - ref| / tol = %.3f" % (C, worst))


# ---- K4b and K7, blocks of padded slices ---------------------------------------------------------------------------------------------
def padded_case(C, nf):
    """(pcm [6 slices][C], ranges [6][2] in values, slice_frames, blocks: list of (start, what)) for blocks of nf frames.  Slice s holds
    noise over its live frames [a, b) and digital silence elsewhere; for stereo the first live frame's left sample and the last one's
    right sample are zero, so that the range in values is odd at both ends"""
    rng = np.random.default_rng(90 + C)
    slice_frames = (nf + SLACK) * F.FRAME
    x = np.zeros((6 * slice_frames, C), np.float32)
    live = [(337 * F.FRAME + 300, 657 * F.FRAME + 500),             # 0: a stretch of 320 frames, its ends inside a frame of most blocks
            (100, slice_frames - 50),                               # 1: nearly everything: covers frame 0 and the last frame of its blocks
            (700 * F.FRAME + 100, 700 * F.FRAME + 300),             # 2: inside one frame | astride two, by the block's start
            (300, 500),                                             # 3: the block's frame 0 alone
            ((nf - 1) * F.FRAME + 300, (nf - 1) * F.FRAME + 500),   # 4: the block's last frame alone
            None]                                                   # 5: nothing but silence
    ranges = np.zeros((6, 2), np.int64)
    for s, ab in enumerate(live):
        if ab is None:
            ranges[s] = (-1, 0)
            continue
        a, b = s * slice_frames + ab[0], s * slice_frames + ab[1]
        v = rng.uniform(-1, 1, (b - a, C)).astype(np.float32)
        v[v == 0] = 0.5
        x[a:b] = v
        if C == 2:
            x[a, 0] = 0
            x[b - 1, 1] = 0
        nz = np.flatnonzero(x[a:b].ravel())
        ranges[s] = (a * C + nz[0], a * C + nz[-1] + 1)             # first value that is not silence, last such value + 1
    # 18 starts a frame apart: the first and the last live frame at every residue of 16; then starts that put a frame's end ON the first
    # live sample and a frame's start ON the last one, and one sample to either side
    blocks = [(k * F.FRAME, "slice 0") for k in range(SLACK)]
    blocks += [(3 * F.FRAME + r, "slice 0") for r in (299, 300, 301, 499, 500, 501)]
    blocks += [(1 * slice_frames + o, "slice 1") for o in (0, 99, 100, SLACK * F.FRAME)]
    blocks += [(2 * slice_frames + o, "slice 2") for o in (0, 150, 100 + 5 * F.FRAME)]
    blocks += [(3 * slice_frames + o, "slice 3") for o in (0, 301, 501, 5 * F.FRAME)]              # ... the last two wholly in the padding
    blocks += [(4 * slice_frames + o, "slice 4") for o in (0, 299, 7 * F.FRAME)]
    blocks += [(5 * slice_frames + 123, "slice 5")]
    return x, ranges, slice_frames, blocks


@pytest.mark.parametrize("C,fpb", ((2, 2), (1, 2), (3, 2), (3, 3)), ids=("stereo", "mono", "three", "three-fpb3"))
def test_frames_edges_padded_slices(gpu, C, fpb):
    """three channels at frames_per_bit 3 are 270 items per bit: more than the wave kernel's tile, K7 runs one thread per bit there --
    the kernel that knows no ranges and loads every cell, so K4b has to write every cell; the same behind the debug switch"""
    awm, ctx, torch = gpu
    key = awm.test_key(7)
    nf = 510 + fpb * F.SOFT_BITS
    wave = fpb * C * 30 <= 256
    x, ranges, slice_frames, blocks = padded_case(C, nf)
    starts = [b for b, _ in blocks]
    try:
        awm.set_params(frames_per_bit=fpb)
        orc.set_params(frames_per_bit=fpb)
        mix = F.mix_entries(key, fpb)
        xd, rd = dev(torch, x), dev(torch, ranges)
        planes, soft, slot = ctx.debug_block_db(key, xd, starts, fill=SENTINEL_BITS, slice_range=rd, slice_frames=slice_frames)
        planes = planes.cpu().numpy()
        if wave and C == 2:
            awm.lib.awm_debug_set_soft_bits_generic(1)
            gplanes, gsoft, gslot = ctx.debug_block_db(key, xd, starts, fill=SENTINEL_BITS, slice_range=rd, slice_frames=slice_frames)
            gplanes = gplanes.cpu().numpy()
    finally:
        awm.lib.awm_debug_set_soft_bits_generic(0)
        awm.set_params()
        orc.set_params()
    assert {0, nf - 1} <= set(mix[:, 0].tolist())                  # (this key's table has items at both edges: the reflected neighbours)
    assert slot.tolist() == list(range(len(blocks)))
    ld = planes.shape[3]
    assert np.isfinite(soft).all()
    if wave and C == 2:
        # the one-thread-per-bit kernel by the switch: no cell of a block left unwritten, the cells the wave kernel's run has as well the
        # same, the soft bits the same
        gw, w = gplanes.view(np.uint32) != SENTINEL_BITS, planes.view(np.uint32) != SENTINEL_BITS
        assert gw[:, :, :, :nf].all() and not gw[:, :, :, nf:].any() and not w.all(axis=(1, 2, 3)).all()
        assert np.array_equal(gplanes.view(np.uint32)[w], planes.view(np.uint32)[w]) and (gplanes[~w & gw] == -96).all()
        assert np.array_equal(gsoft.view(np.uint32), soft.view(np.uint32)) and np.array_equal(gslot, slot)
    worst, seen_lo, seen_hi, shapes = 0.0, set(), set(), set()
    for i, (start, what) in enumerate(blocks):
        what = "%s C=%d block at %d" % (what, C, start)
        first, last = ranges[start // slice_frames]
        lo, hi = F.live_frames(start, nf, C, first, last)
        read = F.cells_read(mix, C, fpb, nf, ld, live=(lo, hi))
        p = planes[i]
        written = p.view(np.uint32) != SENTINEL_BITS
        assert not (read & ~written).any(), (what, "a cell K7 reads is not written", np.argwhere(read & ~written)[:3].tolist())
        assert not written[:, :, nf:].any()
        if not wave:
            assert written[:, :, :nf].all(), (what, "the one-thread-per-bit kernel loads every cell")
        outside = np.ones(ld, bool)
        outside[max(lo, 0):hi + 1] = False
        assert (p[:, :, outside][written[:, :, outside]].view(np.uint32) == np.float32(-96).view(np.uint32)).all(), (what, "padding is not -96")
        want, tol = block_reference(x, start, lo, hi, nf)
        if hi >= lo:
            assert written[:, :, lo:hi + 1].all(), (what, "a live frame is not written")
            worst = max(worst, ratio(np.ascontiguousarray(p[:, :, lo:hi + 1]), np.ascontiguousarray(want[:, :, lo:hi + 1]),
                                     np.ascontiguousarray(tol[:, :, lo:hi + 1]), what))
            seen_lo.add(lo % 16)
            seen_hi.add(hi % 16)
        shapes.add((lo == 0, hi == nf - 1, hi == lo, hi < lo))
        own = F.soft_bits(p, mix, fpb, nf, live=(lo, hi))             # the sentinels left in place: a stray read shows as NaN
        assert np.array_equal(soft[i].view(np.uint32), own.view(np.uint32)), (what, "K7 against its restatement on the device's own planes")
        ref = F.soft_bits(want, mix, fpb, nf)
        sum_tol = F.soft_bits_tol(tol, mix, fpb, nf)
        assert (np.abs(soft[i].astype(np.float64) - ref) <= sum_tol).all(), what
        if hi < lo:
            assert (soft[i].view(np.uint32) == 0).all(), what            # -96 - (-192) / 2, item by item: +0
    assert seen_lo == set(range(16)) and seen_hi == set(range(16)), (seen_lo, seen_hi)
    # (first frame live, last frame live, one live frame, none): frame 0 alone, the last frame alone, every frame, one frame inside, a
    # stretch inside, nothing
    assert {(True, False, True, False), (False, True, True, False), (True, True, False, False), (False, False, True, False),
            (False, False, False, False), (False, False, False, True)} <= shapes, shapes
    print("K4b + K7 padded slices C=%d frames_per_bit %d: %d blocks, largest |got - ref| / tol = %.3f" % (C, fpb, len(blocks), worst))


# ---- K7 alone ------------------------------------------------------------------------------------------------------------------------
def hand_made_planes(seed, n_blocks, C, ld):
    rng = np.random.default_rng(seed)
    shape = (n_blocks, C, F.NB, ld)
    planes = (rng.uniform(-1, 1, shape) * 10.0 ** rng.integers(-6, 4, shape)).astype(np.float32)
    if n_blocks > TINY_BLOCK:
        # one block of odd multiples of 2^-149 below 2^-125: halving such a value is not exact in float32, and the block's sums are
        # exact in double -- 0.5 applied to the neighbours before their float addition shows here and nowhere else
        planes[TINY_BLOCK] = (rng.integers(0, 2 ** 23, shape[1:], dtype=np.uint32) * 2 + 1).view(np.float32) * rng.choice(np.float32([-1, 1]), shape[1:])
    return planes


@pytest.mark.parametrize("fpb", (2, 3))
@pytest.mark.parametrize("C", (2, 1), ids=("stereo", "mono"))
def test_frames_edges_k7_alone(gpu, C, fpb):
    awm, ctx, torch = gpu
    key = awm.test_key(7)
    try:
        awm.set_params(frames_per_bit=fpb)
        orc.set_params(frames_per_bit=fpb)
        mix = F.mix_entries(key, fpb)
        block_frames = 510 + fpb * F.SOFT_BITS
        ld = ctx.block_plane_ld()
        assert ld >= block_frames and ld % 64 == 0 and F.SOFT_BITS % 16 != 0              # (the last wave of a block has n_here < 4)
        planes = hand_made_planes(60 + C + 10 * fpb, 9, C, ld)
        want = np.stack([F.soft_bits(planes[b], mix, fpb, block_frames) for b in range(9)])
        assert np.isfinite(want).all() and len(np.unique(want)) > 9 * 800
        pd = dev(torch, planes)
        # blocks of padded slices: odd and even ranges, bases on and off the frame grid; NaN in every cell K7 has no business reading
        ranges = np.array([(-1, 0), (0, 1), (1000 * F.FRAME * C + 1, 1200 * F.FRAME * C - 1), (1000 * F.FRAME * C, 1200 * F.FRAME * C),
                           (5, 3 * F.FRAME * C), ((block_frames - 2) * F.FRAME * C + 3, 2 ** 33)], np.int64)
        bases = np.array([0, 0, 0, 1, 1023, 2 * F.FRAME + 1, 40 * F.FRAME, 7, 999 * F.FRAME], np.int64)
        which = np.array([2, 3, 0, 2, 3, 4, 5, 1, 2], np.int32)
        live = [F.live_frames(int(bases[b]), block_frames, C, *ranges[which[b]]) for b in range(9)]
        holes = planes.copy()
        for b in range(9):
            holes[b][~F.cells_read(mix, C, fpb, block_frames, ld, live=live[b])] = np.nan
        want_live = np.stack([F.soft_bits(holes[b], mix, fpb, block_frames, live=live[b]) for b in range(9)])
        assert np.isfinite(want_live).all()
        hd = dev(torch, holes)
        got = {}
        for generic in (0, 1):
            awm.lib.awm_debug_set_soft_bits_generic(generic)
            for n in (1, 7, 8, 9):
                got[generic, n] = ctx.debug_soft_bits_planes(key, pd, n_blocks=n)
                assert got[generic, n].shape == (n, F.SOFT_BITS)
            if not generic:                                          # (the one-thread-per-bit kernel knows no ranges: it loads every cell)
                for n in (7, 9):
                    got["live", n] = ctx.debug_soft_bits_planes(key, hd, n_blocks=n, block_base=dev(torch, bases[:n]), slice_range=dev(torch, ranges),
                                                                range_index=dev(torch, which[:n]))
        for n in (1, 7, 8, 9):
            assert np.array_equal(got[0, n].view(np.uint32), want[:n].view(np.uint32)), ("wave kernel against the restatement", n)
            assert np.array_equal(got[1, n].view(np.uint32), got[0, n].view(np.uint32)), ("generic kernel against the wave kernel", n)
        for n in (7, 9):
            assert np.array_equal(got["live", n].view(np.uint32), want_live[:n].view(np.uint32)), ("live ranges", n, live)
    finally:
        awm.lib.awm_debug_set_soft_bits_generic(0)
        awm.set_params()
        orc.set_params()


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_frames_edges_arguments_are_checked_on_the_host(gpu):
    awm, ctx, torch = gpu
    ld = ctx.block_plane_ld()
    n = NF * F.FRAME
    x = torch.zeros((2 * n, 1), dtype=torch.float32, device="cuda")
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    small = torch.zeros((1, 1, F.NB, ld), dtype=torch.float32, device="cuda")
    # accepted: two slices of a block each, one of them silent; nothing to write, soft bits of silence
    planes, soft, slot = ctx.debug_block_db(None, x, [0, n, n + 1], fill=SENTINEL_BITS, slice_range=i64([[-1, 0], [5, 2 * n]]), slice_frames=n)
    assert slot.tolist() == [0, 1, -1] and (soft == 0).all()
    assert (planes[0].cpu().numpy().view(np.uint32) == SENTINEL_BITS).all()
    block_db = (
        dict(indices=[0, n], planes=small),                                                          # a buffer of one block for two
        dict(indices=[0] * 65),
        dict(indices=[]),
        dict(indices=[0], slice_range=i64([[0, 1]])),                                                # ranges without slice_frames
        dict(indices=[0], slice_frames=n),                                                           # ... and the other way round
        dict(indices=[0], slice_range=i64([[0, 1]] * 3), slice_frames=n),                            # three slices in the samples of two
        dict(indices=[0, n], slice_range=i64([[0, 1]]), slice_frames=n),                             # a block behind the last slice
        dict(indices=[0], slice_range=i64([[7, 6], [0, 1]]), slice_frames=n),                        # first > last
        dict(indices=[0], slice_range=i64([[0, 2 * n + 1], [0, 1]]), slice_frames=n),                # last beyond the values
    )
    for kw in block_db:
        with pytest.raises(awm.AwmError):
            ctx.debug_block_db(None, x, kw.pop("indices"), **kw)
    with pytest.raises(awm.AwmError):
        ctx.debug_block_db(None, torch.zeros((n, 4), dtype=torch.float32, device="cuda"), [0])       # four channels
    two = torch.zeros((2, 1, F.NB, ld), dtype=torch.float32, device="cuda")
    assert (ctx.debug_soft_bits_planes(None, two) == 0).all()
    ok = dict(block_base=i64([0, 5]), slice_range=i64([[0, 9], [-1, 0]]), range_index=i32([1, 0]))
    assert (ctx.debug_soft_bits_planes(None, two, **ok) == 0).all()
    k7 = (
        dict(n_blocks=3),                                                                            # more blocks than the planes hold
        dict(n_blocks=0),
        dict(channels=2),                                                                            # ... or more channels
        dict(channels=4),
        dict(ok, block_base=None),                                                                   # the three arrays go together
        dict(ok, range_index=None),
        dict(ok, slice_range=None),
        dict(ok, range_index=i32([1, 2])),                                                           # a slice that is not there
        dict(ok, range_index=i32([-1, 0])),
        dict(ok, block_base=i64([-1, 0])),
        dict(ok, block_base=i64([0, 2 ** 41])),
        dict(ok, slice_range=i64([[9, 8], [-1, 0]])),
        dict(ok, slice_range=i64([[0, 2 ** 42], [-1, 0]])),
    )
    for kw in k7:
        with pytest.raises(awm.AwmError):
            ctx.debug_soft_bits_planes(None, two, **kw)
    # planes of 65 blocks: refused by the count alone
    with pytest.raises(awm.AwmError):
        ctx.debug_soft_bits_planes(None, torch.zeros((65, 1, F.NB, ld), dtype=torch.float32, device="cuda"))
