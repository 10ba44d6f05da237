"""K12 .. K15 (csrc/hip/speed.hip) alone, through their narrowest entry points, at the sizes where their tiling changes -- against the
plain restatements of tests/_speed.py (tied to the oracle by test_speed_restated.py), so that a wrong tile edge cannot hide behind
a tolerance or behind the returned speed.

K12 resample_var_kernel, through ctx.resample_ratio: BIT FOR BIT var_resample32 on the exported table.
  ratios   0.3 (hl 54: table in global memory), 0.49 and 0.625 (the scan's range, table in LDS), 1 / 1.01, 1.25, 2.5, 3.0, 7.3, 1 / 16
           (the smallest legal one, hl 256), 0.1 (hl 160)
  channels 1, 2, 3; stereo on an 8 byte aligned pointer (the <2> form) and one float further (the <0> form), input and output: equal
  lengths  n_out 1, 255, 256, 257, 511, 512, 513 (above ratio 1, where lrint (n_in ratio) skips one, the next length it reaches) and
           an input of hl frames (< one window)
  the long case: stereo, ratio 0.625, n_out = 2 * 4096 * 512 + 2 * 512 + 300: 8195 tiles, two per workgroup, the last workgroup with
           one tile of 300 outputs; restated: the first and last 2 hl outputs, 64 on each side of every 512th tile border and of every
           workgroup border, 20 000 random ones
  modes    awm_debug_set_resample_var_mode 0, 1, 2, 3 give the same bits on every case (1 and 3: the staged window wherever the
           launcher allows it, i.e. stereo, aligned, table in LDS; at 0.1 and 0.3 the table is not in LDS and they run unstaged.  The
           launcher's other condition, span <= 4096, cannot fail while the table fits: 47 taps mean a ratio >= 0.34, a span <= 1600)
  inputs   uniform noise; +-1.0 runs with digital silence at both ends; one impulse per 1000 frames
  The round-up of the phase (ph >= 256) fires at 3.0, for output 3, and at none of the other ratios (see _speed.py: it
  cannot below 2, has no solution at 2.5 and 7.3); every case asserts from the restatement that it fired there and only there.

K13 speed_mags_kernel, through ctx.speed_mags: every value within its derived tolerance of mags64 (var_resample32 (clip)), a
  reference that never touches the device; exactly -96 * 30 * C where every channel is silent.
  rows 129, 100, 65, 64, 63, 48 (ld without padding), 1, 0; channels 1, 2, 3; centres 0.8, 1.0, 1.25; white noise, and at 129 / 100 / 65
  rows a sloped spectrum, a strong tone between bins, channel 1 at 1e-3 and 1e-6 of channel 0, and gaps (both channels; channel 1 only).

K14 speed_compare_kernel, through ctx.speed_scan: BIT FOR BIT compare() on the device's own matrices (ctx.speed_mags of the centre),
  qualities as uint64, speeds exactly; three centres per case (first, middle, last).  Rows 0, 1, 170 and, at 110 s, 18 946 (block 1
  swaps, block 2 contributes: asserted from the restatement's counts).  Steps 1.0007 and 1.02; 1, 3, 5, 7, 9, 11, 13 relative speeds per
  centre (2 n_steps + 1 is odd: the 6 and 12 of a full group never occur as a centre's count, they occur as the groups 6 + 1, 6 + 5,
  6 + 6 + 1).  The launcher has 35 state ranges (pad_start 8908), so its threshold of 1024 workgroups falls at 30 centres for one
  group, 15 for two, 10 for three:
      <1>      3 centres x 1, 5, 13; 1 centre x 3 at 110 s
      <6> z    31 centres x 1, 5; 15 x 7 and 11 x 13 with fold off
      <6> fold 15 centres x 7, 9, 11 (6 + 1, 6 + 3, 6 + 5); 11 x 13 (6 + 6 + 1)
      <12>     wide on, 31 centres x 7, 9, 11
  which form a case takes is asserted by restating the launcher's inequality (_speed.compare_form); every form that can run a case
  gives the same bits.

K15 gather / energy, through ctx.speed_clip_location: equal to orc.speed_clip_location on inputs shorter than the clip, 1 and 5
  candidates, 1 and 3 channels, lengths around 256 * 256 values.

MEASURED on 2026-10-21 (MI355X), largest |got - ref| / tol, for information (the tests print them):
  K13 white: mono 0.113 | stereo 0.0912 | three channels 0.0879;  sloped 0.116 | tone 0.0228 | pair3 0.0148 | pair6 0.057 | gaps 0.112
  K13 against the per-channel oracle on the pairs, in units of the same tolerance: pair3 0.0148 | pair6 0.0570 -- the quiet channel
      does not suffer from riding in the loud one's transform
  K12, K14, K15: equal to the bit.
"""
import numpy as np
import pytest

import _oracle as orc
import _speed as SP

pytestmark = pytest.mark.gpu

KEY = bytes(range(16))
PAYLOAD = "0123456789abcdef0011223344556677"
SPEED_TOL = 2e-6                                 # test_gpu_speed.py's
RATIOS = (0.3, 0.49, 0.625, 1 / 1.01, 1.25, 2.5, 3.0, 7.3, 1 / 16, 0.1)
LENGTHS = (1, 255, 256, 257, 511, 512, 513)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    ctx = awm.Context(0)

    class G:
        pass
    g = G()
    g.torch, g.awm, g.ctx, g.lib = torch, awm, ctx, awm.lib
    g.dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    yield g
    awm.lib.awm_debug_set_resample_var_mode(2)
    awm.lib.awm_debug_set_speed_compare_wide(0)
    awm.lib.awm_debug_set_speed_compare_fold(1)
    ctx.close()


@pytest.fixture(scope="module")
def cols():
    return SP.key_cols(KEY)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- K12 -----------------------------------------------------------------------------------------------------------------------------
def n_in_for(n_out, ratio):
    for n_in in range(max(1, int(n_out / ratio) - 2), int(n_out / ratio) + 3):
        if SP.resample_frames(n_in, ratio) == n_out:
            return n_in
    return None


def offset_view(g, n, C, fill=None):
    """an [n][C] tensor whose pointer is one float past an 8 byte aligned one"""
    flat = g.torch.empty(n * C + 1, dtype=g.torch.float32, device="cuda")
    v = flat[1:].view(n, C)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    if fill is not None:
        v.copy_(fill)
    return v


def k12_all_modes(g, x, ratio):
    """the output of every mode, aligned and (stereo) misaligned: all equal; returns it [n_out][C] float32"""
    xd = g.dev(x)
    assert xd.data_ptr() % 8 == 0
    outs = []
    for mode in (2, 0, 1, 3):
        g.lib.awm_debug_set_resample_var_mode(mode)
        outs.append(g.ctx.resample_ratio(xd, ratio))
        if x.shape[1] == 2:
            outs.append(g.ctx.resample_ratio(offset_view(g, len(x), 2, xd), ratio))                                   # <0>: the input
            outs.append(g.ctx.resample_ratio(xd, ratio, out=offset_view(g, outs[0].shape[0], 2)))                     # <0>: the output
    g.lib.awm_debug_set_resample_var_mode(2)
    for o in outs[1:]:
        assert g.torch.equal(o, outs[0])
    return outs[0].cpu().numpy()


def k12_check(g, x, ratio, outputs=None, got=None):
    geo = SP.VarGeometry(ratio)
    tab = g.awm.binding.var_resample_table(ratio)
    n_out = SP.resample_frames(len(x), ratio)
    if got is None:
        got = k12_all_modes(g, x, ratio)
    assert got.shape == (n_out, x.shape[1])
    info = {}
    want = SP.var_resample32(x, tab, geo.hl, ratio, n_out, outputs, info=info)
    assert (info["round_ups"] > 0) == (ratio == 3.0 and n_out > 3), info               # var_phase's ph >= 256: output 3 at 3.0
    sel = got if outputs is None else got[outputs]
    assert bits_equal(sel, want), (ratio, x.shape, int((sel.view(np.uint32) != want.view(np.uint32)).sum()))
    return n_out


@pytest.mark.parametrize("C", (1, 2, 3))
@pytest.mark.parametrize("ratio", RATIOS)
def test_k12_lengths(gpu, ratio, C):
    geo = SP.VarGeometry(ratio)
    for n_out in LENGTHS:
        while n_in_for(n_out, ratio) is None:                    # (ratios above 1 skip lengths: the next one they reach)
            n_out += 1
        assert k12_check(gpu, SP.k12_inputs(n_in_for(n_out, ratio), C, "noise", n_out), ratio) == n_out
    x = SP.k12_inputs(geo.hl, C, "noise", 3)                     # shorter than one window: every tap pair has a zero side
    assert len(x) < 2 * geo.hl and k12_check(gpu, x, ratio) == SP.resample_frames(geo.hl, ratio)


def test_k12_every_length_is_covered():
    assert all(all(n_in_for(n, r) is not None for n in LENGTHS) for r in RATIOS if r <= 1)


@pytest.mark.parametrize("kind", ("runs", "impulses"))
@pytest.mark.parametrize("ratio", RATIOS)
def test_k12_inputs(gpu, ratio, kind):
    n_in = int((5000 if ratio > 0.1 else 1200) / ratio)
    for C in (2, 3):
        x = SP.k12_inputs(n_in, C, kind, 7)
        k12_check(gpu, x, ratio)
        assert kind != "runs" or not x[:100].any()


def test_k12_tile_loop(gpu):
    ratio, tile, per_wg = 0.625, 512, 2
    geo = SP.VarGeometry(ratio)
    n_out = 2 * 4096 * tile + 2 * tile + 300
    n_tiles = (n_out + tile - 1) // tile
    assert n_tiles == 8195 and min(16, max(1, n_tiles // 4096)) == per_wg and n_tiles % per_wg == 1       # launch_resample_var's choice
    n_in = n_in_for(n_out, ratio)
    x = SP.k12_inputs(n_in, 2, "noise", 99)
    around = np.arange(-64, 64)
    borders = np.concatenate([np.arange(tile * 512, n_out, tile * 512), np.arange(tile * per_wg, n_out, tile * per_wg)])
    outputs = np.concatenate([np.arange(2 * geo.hl), np.arange(n_out - 2 * geo.hl, n_out), (borders[:, None] + around[None, :]).ravel(),
                              np.random.default_rng(5).integers(0, n_out, 20000)])
    outputs = np.unique(outputs[(outputs >= 0) & (outputs < n_out)])
    assert n_out - 1 in outputs and (n_tiles - 1) * tile - 1 in outputs and (n_tiles - 1) * tile in outputs
    xd = gpu.dev(x)
    outs = []
    for mode in (2, 0, 1, 3):
        gpu.lib.awm_debug_set_resample_var_mode(mode)
        outs.append(gpu.ctx.resample_ratio(xd, ratio))
    gpu.lib.awm_debug_set_resample_var_mode(2)
    outs.append(gpu.ctx.resample_ratio(offset_view(gpu, n_in, 2, xd), ratio))                                         # <0>
    for o in outs[1:]:
        assert gpu.torch.equal(o, outs[0])
    k12_check(gpu, x, ratio, outputs, got=outs[0].cpu().numpy())


# ---- K13 -----------------------------------------------------------------------------------------------------------------------------
def k13_case(g, cols, x, xd, loc, center, rows, extra=77):
    """(largest |got - ref| / tol, got, ref, tol) of one centre's matrix; asserts the row count and the exact values"""
    C = x.shape[1]
    seconds = SP.seconds_for_rows(rows, center, extra)
    start, n_in, n_out, n_rows = SP.mags_geometry(len(x), loc, center, seconds)
    assert n_rows == rows and start + n_in <= len(x)
    got = g.ctx.speed_mags(KEY, xd, loc, center, seconds)
    assert got.shape == (rows, 510, 2)
    if rows == 0:
        return 0.0, got, got, None
    ratio = center / 2
    geo = SP.VarGeometry(ratio)
    sub = SP.var_resample32(x[start:start + n_in], g.awm.binding.var_resample_table(ratio), geo.hl, ratio, n_out)
    ref, tol = SP.mags64(sub, cols)
    exact = tol == 0
    assert bits_equal(got[exact], ref[exact])
    if exact.all():
        return 0.0, got, ref, tol
    return float((np.abs(got.astype(np.float64) - ref)[~exact] / tol[~exact]).max()), got, ref, tol


@pytest.mark.parametrize("C", (1, 2, 3))
def test_k13_rows_and_centres(gpu, cols, C):
    x = np.ascontiguousarray(SP.materials()["white"][:, :C])
    xd = gpu.dev(x)
    worst = 0.0
    for rows in (129, 100, 65, 64, 63, 48, 1, 0):                # (the largest first: the scratch matrix never grows afterwards)
        for center, loc in ((0.8, 0.37), (1.0, 0.0), (1.25, 0.11)):
            r, got, _, _ = k13_case(gpu, cols, x, xd, loc, center, rows, extra=0 if rows in (64, 1) else 77)
            worst = max(worst, r)
            assert r <= 1, (rows, center, r)
    print("K13 white, %d channels: largest |got - ref| / tol %.3g" % (C, worst))


@pytest.mark.parametrize("name", ("sloped", "tone", "pair3", "pair6", "gaps"))
def test_k13_materials(gpu, cols, name):
    m = SP.materials()[name]
    worst = 0.0
    for C in (2, 3):
        x = np.ascontiguousarray(m[:, :C])
        xd = gpu.dev(x)
        for center, rows, loc in ((0.8, 129, 0.37), (1.0, 100, 0.2), (1.25, 65, 0.0)):
            r, got, ref, tol = k13_case(gpu, cols, x, xd, loc, center, rows)
            worst = max(worst, r)
            if name == "gaps":
                silent = (tol == 0).all(axis=(1, 2))
                assert silent.sum() >= 5 and (got[silent] == np.float32(-96 * 30 * C)).all()
                if center == 0.8:                                # channel 1 (and 2) alone silent: exactly -96 per band from them
                    assert (~silent[:, None, None] & (ref < -96 * 30 * (C - 1))).any()
            if name.startswith("pair"):
                seconds = SP.seconds_for_rows(rows, center, 77)
                o = orc.speed_mags(KEY, x, C, loc, center, seconds)
                print("K13 %s, %d channels, centre %.2f: largest |got - per-channel oracle| / tol %.3g" %
                      (name, C, center, float((np.abs(got.astype(np.float64) - o) / tol).max())))
            assert r <= 1, (C, center, r)
    print("K13 %s: largest |got - ref| / tol %.3g" % (name, worst))


# ---- K14 -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replayed(gpu):
    """marked noise replayed at 1.01 (the oracle's resampler), long enough for the 110 s scan: (host, device)"""
    y = orc.add(KEY, orc.gen_noise(KEY, 146 * 44100 * 2), 2, PAYLOAD)
    z = orc.resample_ratio(y, 2, 1 / 1.01).reshape(-1, 2)
    return z, gpu.dev(z)


def k14_forms(n_centers, per):
    """the (wide, fold) settings that lead to different launches of this case, with the form each takes"""
    out = {}
    for wide, fold in ((0, 1), (0, 0), (1, 1)):
        out.setdefault(SP.compare_form(n_centers, per, wide, fold), (wide, fold))
    return out


def k14_case(g, cols, zd, loc, seconds, step, n_steps, n_center_steps, want_forms, stats=None):
    centers = SP.scan_centers([1.01], step, n_steps, n_center_steps)
    per = 2 * n_steps + 1
    forms = k14_forms(len(centers), per)
    assert sorted(forms) == sorted(want_forms), (forms, want_forms)
    results = []
    for form, (wide, fold) in forms.items():
        g.lib.awm_debug_set_speed_compare_wide(wide)
        g.lib.awm_debug_set_speed_compare_fold(fold)
        results.append(g.ctx.speed_scan(KEY, zd, loc, seconds, step, n_steps, n_center_steps, [1.01]))
    g.lib.awm_debug_set_speed_compare_wide(0)
    g.lib.awm_debug_set_speed_compare_fold(1)
    s, q = results[0]
    for s2, q2 in results[1:]:
        assert bits_equal(s2, s) and bits_equal(q2, q)
    assert len(s) == len(centers) * per and (np.diff(s) >= 0).all()
    by_speed = dict(zip(s.tolist(), q.tolist()))
    rows = []
    for c in sorted({0, len(centers) // 2, len(centers) - 1}):
        m = g.ctx.speed_mags(KEY, zd, loc, centers[c], seconds)
        rows.append(len(m))
        rel, reported = SP.rel_speeds(centers[c], step, n_steps)
        want = SP.compare(m, len(m), rel, 0.01, cols, stats)
        for sp, w in zip(reported, want):
            if w > 0:
                assert sp in by_speed and np.float64(by_speed[sp]).view(np.uint64) == np.float64(w).view(np.uint64), (c, sp, by_speed.get(sp), w)
            else:
                assert sp not in by_speed                            # (reported as { 0, 0 })
    return s, q, rows


K14_CASES = [                                                    # step, n_steps, n_center_steps, forms
    (1.02, 0, 1, ["<1>"]), (1.02, 2, 1, ["<1>"]), (1.02, 6, 1, ["<1>"]), (1.0007, 6, 1, ["<1>"]),
    (1.0007, 0, 15, ["<6>z"]), (1.0007, 2, 15, ["<6>z"]),
    (1.0007, 3, 7, ["<6>fold", "<6>z"]), (1.0007, 4, 7, ["<6>fold", "<6>z"]), (1.0007, 5, 7, ["<6>fold", "<6>z"]), (1.0007, 6, 5, ["<6>fold", "<6>z"]),
    (1.0007, 3, 15, ["<12>", "<6>fold", "<6>z"]), (1.0007, 4, 15, ["<12>", "<6>fold", "<6>z"]), (1.0007, 5, 15, ["<12>", "<6>fold", "<6>z"]),
]


@pytest.mark.parametrize("step,n_steps,n_center_steps,forms", K14_CASES)
def test_k14_forms_at_170_rows(gpu, cols, replayed, step, n_steps, n_center_steps, forms):
    z, zd = replayed
    seconds = SP.seconds_for_rows(170, 1.01)
    s, q, rows = k14_case(gpu, cols, zd, 0.3, seconds, step, n_steps, n_center_steps, forms)
    assert all(160 <= r <= 180 for r in rows) and (q > 0).all()


@pytest.mark.parametrize("rows", (0, 1))
def test_k14_no_row_and_one_row(gpu, cols, replayed, rows):
    z, zd = replayed
    for step, n_steps, n_center_steps, forms in ((1.02, 2, 1, ["<1>"]), (1.0007, 3, 7, ["<6>fold", "<6>z"]), (1.0007, 3, 15, ["<12>", "<6>fold", "<6>z"])):
        centers = SP.scan_centers([1.01], step, n_steps, n_center_steps)
        seconds = SP.seconds_for_rows(rows, centers[len(centers) // 2])
        assert max(SP.mags_geometry(len(z), 0.3, c, seconds)[3] for c in centers) == rows          # (1: some centres have 1 row, some none)
        if rows == 0:
            for wide, fold in k14_forms(len(centers), 2 * n_steps + 1).values():
                gpu.lib.awm_debug_set_speed_compare_wide(wide)
                gpu.lib.awm_debug_set_speed_compare_fold(fold)
                s, q = gpu.ctx.speed_scan(KEY, zd, 0.3, seconds, step, n_steps, n_center_steps, [1.01])
                assert len(s) == len(centers) * (2 * n_steps + 1) and not s.any() and not q.any()              # every score { 0, 0 }
            gpu.lib.awm_debug_set_speed_compare_wide(0)
            gpu.lib.awm_debug_set_speed_compare_fold(1)
        else:
            k14_case(gpu, cols, zd, 0.3, seconds, step, n_steps, n_center_steps, forms)


def test_k14_three_blocks(gpu, cols, replayed):
    """110 s: more than 17808 rows, so that block 1 (up and down swapped) and block 2 contribute"""
    z, zd = replayed
    stats = {}
    s, q, rows = k14_case(gpu, cols, zd, 0.3, 110.0, 1.0007, 1, 0, ["<1>"], stats)
    counts = np.array(stats["block_counts"])
    assert rows[0] > 17808 and (counts > 0).all()                # every relative speed has states that count block 2 columns
    assert q.max() > 1 and abs(s[q.argmax()] - 1.01) < 2e-3      # a real peak
    stats = {}
    s, q, rows = k14_case(gpu, cols, zd, 0.3, 110.0, 1.0007, 3, 7, ["<6>fold", "<6>z"], stats)
    assert min(rows) > 17808 and (np.array(stats["block_counts"]) > 0).all()


# ---- K15 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (1, 3))
def test_k15_clip_location(gpu, C):
    parts = 256 * 256                                            # ENERGY_PARTS workgroups of 256 threads: one value per thread
    lengths = [parts // C - 1, parts // C, parts // C + 1, (parts + 255) // C, 2 * parts // C + 3, 5000, 300000]
    for i, n in enumerate(lengths):
        x = np.random.default_rng(100 + i).uniform(-1, 1, (n, C)).astype(np.float32)
        x[: n // 3] *= np.float32(0.25)                          # the candidates' energies differ
        xd = gpu.dev(x)
        for seconds in (25.0, 0.4, n / 44100 * 0.5):             # longer than the input (start_sec < 0), shorter
            for candidates in (1, 5):
                want = orc.speed_clip_location(KEY, x, C, seconds, candidates)
                assert gpu.ctx.speed_clip_location(KEY, xd, seconds, candidates) == want, (n, seconds, candidates)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_detect_speed_on_a_quiet_channel_beside_a_loud_one(gpu):
    x = orc.gen_noise(KEY, 20 * 44100 * 2).reshape(-1, 2) * np.array([1, 1e-3], np.float32)
    z = orc.resample_ratio(orc.add(KEY, x, 2, PAYLOAD), 2, 1 / 1.01).reshape(-1, 2)
    use, best, quality = gpu.ctx.detect_speed(KEY, gpu.dev(z))
    o_use, o_best, o_quality = orc.detect_speed(KEY, z, 2)
    print("detect_speed on pair3: %.7f (quality %.4f), oracle %.7f (%.4f)" % (best, quality, o_best, o_quality))
    assert (use is None) == (o_use is None) and abs(best - o_best) <= SPEED_TOL and abs(best - 1.01) < 1e-3
