"""K4s (csrc/hip/kernels.hip, launch_sync_db_sliding) held to a float64 transform, value by value, in the layout the product runs it
in: gathered rows through awm_debug_sync_db_sliding_rows_d, which fills SyncDbArgs as SyncFinder's refinement does.

The yardstick is tests/_sliding.py::ref_db (float64 rfft, analytic von Hann window, the reference's last float steps), which
test_sliding_restated.py ties to the oracle's sync_fft on the CPU; the tolerance is ref_db's own, derived per value:
sensitivity to one float32 ulp in re and im + K ulp32 (|value|), K = 4 (_sliding.K_ULPS), no value excluded.  have flags, -96 / -192,
the +0 of skipped offsets and the sentinels are exact.

    stereo   sync_db_sliding4_kernel (form 4, the default), ld = 64 with the 65th offset in the tail array
    mono     sync_db_sliding_kernel<1>, ld = 72, no tail
    forms 0 and 3 in the gathered layout (ld = 72) equal form 4 bit for bit
    form 4 through awm_debug_sync_db_sliding_d (the bands layout of test_refinement_kernel_forms) against ref_db as well

Every out / tail / have buffer is prefilled with a sentinel (a NaN bit pattern; 0x7f) and has one plane more than the streams fill: a
cell the kernel has no business writing must still hold it -- columns >= count, the tail of a stream of at most 64 offsets,
have[count..], all of a stream with count 0, the slots of a partial plane beyond n_streams.  (The dB cells of a row that is skipped as a
whole are the kernel's to leave: only have = 0 is asserted there.)  The PCM carries 2048 frames of NaN behind the n_frames passed in.
The cases -- layout, counts, ends of the buffer, zero rules, levels, skip rules -- are _sliding.cases().

K = 4 is in force and did not have to move.  Measured on an MI355X on 2026-10-18 (each test prints its figure): the largest difference
beyond a value's sensitivity term was 2.81 ulp32 (stereo, the gaps case), 1.98 ulp32 in every other case, 1.96 ulp32 mono."""
import numpy as np
import pytest

import _sliding as S

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7fc0dead], np.uint32).view(np.float32)[0]
SENTINEL_BITS = 0x7fc0dead
HAVE_SENTINEL = 0x7f
CASES = {c.name: c for c in S.cases()}
_wanted = {}


def wanted(name, C):
    """the reference of a case in the kernel's layout, computed once and shared"""
    if (name, C) not in _wanted:
        case = CASES[name]
        _wanted[name, C] = S.gathered(case, C, (case.n_planes + 1) * case.rpp)
    return _wanted[name, C]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    ctx = awm.Context(0)
    yield awm, ctx, torch
    awm.lib.awm_debug_set_refine_form(4)
    ctx.close()


def device_pcm(torch, case, C):
    x = np.concatenate([case.pcm[:, :C], np.full((2048, C), np.nan, np.float32)])
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def launch(gpu, case, C, form, ld, with_tail):
    """(dB [slots][60][65] float32 with the sentinel where nothing was written, have [slots][65] int8) of one launch; asserts that
    the columns 65 .. ld - 1 (or the tail's second column) still hold the sentinel"""
    awm, ctx, torch = gpu
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n_slots = (case.n_planes + 1) * case.rpp
    out = torch.full((n_slots, S.ROWS, ld), float("nan"), dtype=torch.float32, device="cuda")
    out.view(torch.int32).fill_(SENTINEL_BITS)
    tail = None
    if with_tail:
        tail = torch.empty((n_slots, S.ROWS + 4), dtype=torch.float32, device="cuda")
        tail.view(torch.int32).fill_(SENTINEL_BITS)
    have = torch.full((n_slots, 72), HAVE_SENTINEL, dtype=torch.int8, device="cuda")
    sliced = case.slice_of is not None
    ranges = None
    if case.ranges is not None:
        # the range of every slice as the kernel is to see it (any stream of the slice gives it)
        ranges = np.zeros((case.n_slices, 2), np.int64)
        for s in range(len(case.bases)):
            ranges[case.slice(s)] = case.range_values(s, C)
    first, last = case.range_values(0, C) if case.ranges is None else (0, 0)
    awm.lib.awm_debug_set_refine_form(form)
    try:
        ctx.sync_db_sliding_rows(device_pcm(torch, case, C), len(case.pcm), dev(case.bases), dev(case.counts), int(case.counts.max()), case.rpp,
                                 dev(case.perm), dev(case.pos), first, last, out, have, tail=tail,
                                 stream_range=dev(ranges) if ranges is not None else None, range_index=dev(case.slice_of) if sliced else None,
                                 range_div=case.rpp, tables_per_slice=1 if sliced else 0)
    finally:
        awm.lib.awm_debug_set_refine_form(4)
    out, have = out.cpu().numpy(), have.cpu().numpy()
    db = np.full((n_slots, S.ROWS, 65), SENTINEL, np.float32)
    db[:, :, :min(ld, 65)] = out[:, :, :65]
    assert (out[:, :, 65:].view(np.uint32) == SENTINEL_BITS).all()
    if with_tail:
        tail = tail.cpu().numpy()
        assert (tail[:, S.ROWS:].view(np.uint32) == SENTINEL_BITS).all()
        if ld > 64:
            assert (out[:, :, 64].view(np.uint32) == SENTINEL_BITS).all()
        db[:, :, 64] = tail[:, :S.ROWS]
    assert (have[:, 65:] == HAVE_SENTINEL).all()
    return db, have[:, :65]


def check(db, have, want, tol, written, have_want, loose, what):
    """every cell against the reference: written ones within their tolerance (exact where it is 0), all others the sentinel"""
    bits = db.view(np.uint32)
    strict = ~loose[:, None, None]
    stale = ~written & strict & (bits != SENTINEL_BITS)
    assert not stale.any(), (what, "written where nothing belongs", np.argwhere(stale)[:5].tolist())
    with np.errstate(invalid="ignore"):
        d = np.abs(db.astype(np.float64) - want)
        bad = written & ~(d <= tol)                                  # (a NaN -- an unwritten cell, an over-read -- is bad)
    zero = written & (tol == 0)
    bad |= zero & (bits != want.view(np.uint32))                  # -96, -192 and +0 to the bit (+0, not -0)
    if bad.any():
        i = np.argwhere(bad)
        worst = np.nanmax(np.where(bad & (tol > 0), d / np.where(tol > 0, tol, 1), 0))
        raise AssertionError("%s: %d of %d values off, worst %.3g x its tolerance, first (slot, row, offset) %s got %r want %r tol %.3g"
                             % (what, len(i), int(written.sum()), worst, i[0].tolist(), db[tuple(i[0])], want[tuple(i[0])], tol[tuple(i[0])]))
    have_want = np.where(have_want < 0, HAVE_SENTINEL, have_want)
    assert np.array_equal(have, have_want), (what, "have flags", np.argwhere(have != have_want)[:5].tolist())
    k = written & (tol > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ulps = np.where(k, (d - (tol - S.K_ULPS * S.ulp32(want))) / S.ulp32(want), 0)
    print("%s: %d values, %d exact by rule; beyond the sensitivity term at most %.2f ulp32 of K = %d"
          % (what, int(written.sum()), int(zero.sum()), max(float(ulps.max()), 0.0), S.K_ULPS))


@pytest.mark.parametrize("name", list(CASES))
def test_stereo_product_kernel(gpu, name):
    """form 4, ld = 64 + tail: sync_db_sliding4_kernel as the refinement launches it"""
    db, have = launch(gpu, CASES[name], 2, 4, 64, True)
    check(db, have, *wanted(name, 2), "%s stereo" % name)


@pytest.mark.parametrize("name", list(CASES))
def test_mono_kernel(gpu, name):
    """sync_db_sliding_kernel<1>, ld = 72, the 65th offset in the row"""
    db, have = launch(gpu, CASES[name], 1, 4, 72, False)
    check(db, have, *wanted(name, 1), "%s mono" % name)


@pytest.mark.parametrize("name", list(CASES))
def test_forms_0_and_3_equal_form_4_in_the_gathered_layout(gpu, name):
    """ld = 72 without a tail for all three: the same bits in every cell the reference says is written, the same have flags, the
    sentinel elsewhere; and form 4 with the row's 65th value in the row equals form 4 with the tail"""
    _, _, written, _, loose = wanted(name, 2)
    f4, h4 = launch(gpu, CASES[name], 2, 4, 72, False)
    t4, th4 = launch(gpu, CASES[name], 2, 4, 64, True)
    strict = ~loose[:, None, None]
    assert np.array_equal(f4.view(np.uint32)[strict & written], t4.view(np.uint32)[strict & written]) and np.array_equal(h4, th4)
    for form in (0, 3):
        f, h = launch(gpu, CASES[name], 2, form, 72, False)
        same = f.view(np.uint32) == f4.view(np.uint32)
        assert same[np.broadcast_to(strict, same.shape)].all(), (form, np.argwhere(~same & strict)[:5].tolist())
        assert np.array_equal(h, h4), form


def test_form_4_in_the_bands_layout(gpu):
    """the kernel test_refinement_kernel_forms compares the other forms with (sync_db_sliding4_bands_kernel through
    awm_debug_sync_db_sliding_d, count = 65, all 81 bands) against ref_db: anchors those equalities"""
    awm, ctx, torch = gpu
    case = CASES["gaps"]
    pick = np.arange(0, len(case.bases), 3)
    awm.lib.awm_debug_set_refine_form(4)
    x = torch.from_numpy(case.pcm).cuda()
    got = ctx.sync_db_sliding(x, case.bases[pick], 65).cpu().numpy()                    # [stream][81][72]
    assert (got[:, :, 65:] == 0).all()
    want = np.zeros((len(pick), S.NB, 65), np.float32)
    tol = np.zeros((len(pick), S.NB, 65))
    for i, s in enumerate(pick):
        db, hv, tl = S.ref_db(case.pcm, int(case.bases[s]), 65)
        assert hv.all()
        want[i], tol[i] = db.T, tl.T
    with np.errstate(invalid="ignore"):
        d = np.abs(got[:, :, :65].astype(np.float64) - want)
        bad = ~(d <= tol) | ((tol == 0) & (got[:, :, :65].view(np.uint32) != want.view(np.uint32)))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), float(np.nanmax(d / np.maximum(tol, 1e-30) * (tol > 0))))
    assert (tol == 0).any()


def test_arguments_are_checked_on_the_host(gpu):
    """what the kernels take on trust is refused before a launch: counts beyond 65 or beyond count0, rows of 64 without a tail, a
    tail for mono, a window past n_frames, a negative base"""
    awm, ctx, torch = gpu
    x = torch.zeros((4096, 2), dtype=torch.float32, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    perm, pos = S.random_tables(np.random.default_rng(1), 1, 1)
    perm, pos = torch.from_numpy(perm).cuda(), torch.from_numpy(pos).cuda()

    def call(base, count, count0, ld, tail, pcm=x, n_frames=4096):
        out = torch.zeros((1, S.ROWS, ld), dtype=torch.float32, device="cuda")
        have = torch.zeros((1, 72), dtype=torch.int8, device="cuda")
        tl = torch.zeros((1, S.ROWS), dtype=torch.float32, device="cuda") if tail else None
        ctx.sync_db_sliding_rows(pcm, n_frames, torch.tensor([base], dtype=torch.int64, device="cuda"), i32([count]), count0, 1, perm, pos,
                                 0, 2 * n_frames, out, have, tail=tl)
        return out, have

    out, have = call(4096 - 1024 - 8 * 64, 65, 65, 64, True)               # the largest stream that fits: accepted, all silence
    assert (out == -192).all() and (have[0, :65] == 1).all()
    for bad in ((0, 66, 66, 72, False), (0, 3, 2, 72, False), (0, 65, 65, 64, False), (4096 - 1024 - 8 * 64 + 1, 65, 65, 72, False),
                (-1, 1, 1, 72, False), (0, 1, 1, 72, True, x[:, :1].contiguous()), (0, -1, 1, 72, False), (0, 1, 1, 72, False, x, 1023)):
        with pytest.raises(awm.AwmError):
            call(*bad)
