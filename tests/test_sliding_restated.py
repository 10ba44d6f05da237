"""tests/_sliding.py::ref_db -- the float64 transform test_gpu_sliding_edges.py holds K4s to -- tied to the oracle's sync_fft
(oracle/awm_oracle.cc, the restatement of the reference's syncfinder.cc:560-605) on the CPU, so that the GPU test's yardstick is
not its author's opinion.  CPU only.

On a few streams of every case of _sliding.cases(), stereo and mono, offset by offset (sync_fft of one frame at base + 8 o with
the case's first / last): the have flags are equal, -96 / -192 and the +0 of a skipped offset are equal to the bit wherever
ref_db's rules fire, and the dB values are close.  How close is not ref_db's tolerance: the oracle windows in the TIME domain with
the reference's float-rounded table, ref_db with the analytic window in double -- two definitions that part on bins which fall far
below their window's mean by chance, and on windows of which only the outermost samples are left.  OBSERVED holds the largest
difference over exactly these streams; the test asserts twice that.

Two more facts the GPU test leans on: the oracle's window table IS the analytic window rounded to float32 (entry 0 exactly 0: the
rule "a window with nothing behind position 0 is a frame of zeros" rests on it), and ref_db's tolerance is finite, and its
per-channel values <= 0, on every value of the case list."""
import numpy as np
import pytest

import _oracle as orc
import _sliding as S

CASES = {c.name: c for c in S.cases()}
PER_CASE = 12                            # streams per case and channel count, spread evenly over the case's list

# max |oracle - ref_db| in dB over the compared streams of all cases, measured on 2026-10-18 (x86-64, numpy's pocketfft): 9.92e-5 dB,
# stereo and mono alike (in the cases "layout" and "counts"; the other cases: 6.1e-5 stereo and 6.9e-5 mono in the gaps, 6.1e-5 on the
# levels, 4.6e-5 and 2.3e-5 under the skip rules).  The test asserts twice the maximum.
OBSERVED = 9.92e-5


def picked(case):
    live = np.flatnonzero(case.counts > 0)
    return live[np.unique(np.linspace(0, len(live) - 1, PER_CASE).astype(int))]


@pytest.mark.parametrize("C", (2, 1), ids=("stereo", "mono"))
@pytest.mark.parametrize("name", list(CASES))
def test_ref_db_against_the_oracle(name, C):
    case = CASES[name]
    x = np.ascontiguousarray(case.pcm[:, :C])
    worst, n_exact, n_values = 0.0, 0, 0
    for s in picked(case):
        base, count = int(case.bases[s]), int(case.counts[s])
        first, last = case.range_values(s, C)
        if first < 0:
            first = last = x.size + 1                                  # nothing but silence: every frame ends before `first`
        db, have, tol = S.ref_db(x, base, count, first, last)
        for o in range(count):
            odb, ohave = orc.sync_fft(x, C, base + S.HOP * o, 1, None, first, last)
            assert int(ohave[0]) == int(have[o]), (s, o)
            exact = tol[o] == 0
            assert np.array_equal(odb[0][exact].view(np.uint32), db[o][exact].view(np.uint32)), (s, o)
            if not exact.all():
                worst = max(worst, float(np.abs(odb[0].astype(np.float64) - db[o])[~exact].max()))
            n_exact += int(exact.sum())
            n_values += S.NB
    print("%s %s: %d values, %d exact by rule, max |oracle - ref_db| = %.3g dB" % (name, "stereo" if C == 2 else "mono", n_values, n_exact, worst))
    assert worst <= 2 * OBSERVED, worst
    if name in ("gaps", "skip", "skip-slices"):
        assert n_exact > 0


def test_the_oracle_window_is_the_analytic_window():
    w = orc.window(S.FRAME)
    assert w.dtype == np.float32 and np.array_equal(w, S.WINDOW.astype(np.float32))
    assert w[0] == 0 and (w[1:] > 0).all() and abs(float(w.astype(np.float64).sum()) - 2) < 1e-8


def test_tolerance_is_finite_and_values_are_negative():
    """over every value of the case list: the sensitivity term is finite (a denormal or zero abs2 included) and no channel's dB
    value is positive -- what `K ulp32 (|sum|)` bounds the parts' rounding with"""
    n = 0
    for case in CASES.values():
        for s in np.flatnonzero(case.counts > 0):
            parts, sens, fired = S.channel_parts(case.pcm, int(case.bases[s]), int(case.counts[s]))
            assert np.isfinite(sens).all() and np.isfinite(parts).all() and (parts <= 0).all(), (case.name, s)
            assert (sens[fired] == 0).all() and (parts[fired] == -96).all()
            n += parts.size
    assert n > 2 * 81 * 65 * 300
