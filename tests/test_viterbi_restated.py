"""The numpy restatement of conv_decode_soft (tests/_viterbi.py) pinned to the oracle and, where it is built, to the compiled
reference -- bit for bit: decoded bits, and the error value as a float32 bit pattern.  CPU only.

test_gpu_viterbi_edges.py holds K8 to the values stored in tests/golden/viterbi_edges.npz.  What makes those inputs worth
storing is decided by the restatement (a merged decision on the survivor path, ties on the survivor path, ...), so every
condition the fixture was built under is checked again here on the stored file: a fixture that stops telling the reference from
a decoder without the repeat path, or from one that hands ties to the high predecessor, fails here, without a GPU.

A decode costs 0.1 - 0.5 s in the restatement; every stored input is decoded once (module fixture) and shared."""
import os

import numpy as np
import pytest

import _oracle as orc
import _ref
import _viterbi as V

HERE = os.path.dirname(os.path.abspath(__file__))
N = 143
TIES = ("tie:all-0.5", "tie:hard, 10% flipped", "tie:hard, 30% flipped", "tie:quarters", "tie:half erased", "tie:flat 1e-6", "tie:flat 3e-7")
MAGNITUDES = ("mag:offset 100", "mag:1e-3 about 0.5", "mag:+-1e+19", "mag:+-3e+38", "mag:-0.0 and denormals")
NAN_INF = ("nan:index 0 only", "nan:index 1", "nan:last step", "nan:step 20", "inf:single +inf", "inf:+inf and -inf in one step")


@pytest.fixture(scope="module")
def edges():
    groups, empty = V.load_edges(os.path.join(HERE, "golden", "viterbi_edges.npz"))
    model = {key: [V.decode(key[0], x, classes=name.startswith(("steered", "tie:"))) for name, x, _, _, _ in items]
             for key, items in groups.items()}
    return groups, empty, model


def pinned(bt, x, r):
    for mod in (orc, _ref) if _ref.available() else (orc,):
        bits, err = mod.conv_decode_soft(bt, x)
        assert np.array_equal(bits, r.bits) and V.same_float(err, r.error), (mod.__name__, bt, err, r.error)


def test_every_fixture_input(edges):
    groups, _, model = edges
    assert sorted(groups) == sorted([(bt, N) for bt in (0, 1, 2)] + [(bt, n) for bt in (0, 2) for n in V.LENGTHS])
    for (bt, n), items in groups.items():
        for (name, x, bits, err, _), r in zip(items, model[(bt, n)]):
            assert x.dtype == np.float32 and x.size == n * V.rate(bt) and bits.size == n - V.ORDER
            assert np.array_equal(bits, r.bits) and V.same_float(err, r.error), (bt, n, name)      # what is stored
            pinned(bt, x, r)                                                                            # and what it was stored from


@pytest.mark.parametrize("bt", [0, 1, 2])
def test_fresh_gaussian_inputs(bt):
    rng = np.random.default_rng(300 + bt)
    for n in (N,) + V.LENGTHS:
        x = V.gaussian(bt, rng, n, float(rng.choice([0.3, 0.7, 1.5])))
        pinned(bt, x, V.decode(bt, x, classes=False))


@pytest.mark.parametrize("bt", [0, 1, 2])
def test_steered_merges(edges, bt):
    """each steered input: the decision (t, m) is a merged one, the survivor runs through it, and the decoder without the repeat
    path returns other bits; at least 6 per code type, at most one empty cell, and the fixture names the cell it left empty"""
    groups, empty, model = edges
    filled = np.zeros(len(V.CELLS), int)
    for (name, x, bits, _, (t, m)), r in zip(groups[(bt, N)], model[(bt, N)]):
        if name != "steered":
            assert (t, m) == (-1, -1)
            continue
        assert V.cell_of(t) is not None and r.path[t] == m and r.cls[t, m] == V.MERGED and r.on_path["merged"] >= 1, (t, m)
        assert not np.array_equal(r.bits_merge_blind, bits), (t, m)
        # the clean tail: the survivor costs nothing after step t
        assert np.all(np.isin(x[(t + 1) * V.rate(bt):], (0.0, 1.0)))
        filled[V.cell_of(t)] += 1
    assert filled.sum() >= 6 and np.count_nonzero(filled == 0) <= 1, filled
    assert sorted(e for e in empty if e.startswith(V.TYPES[bt] + ":")) == sorted("%s: %s" % (V.TYPES[bt], V.CELLS[c]) for c in np.flatnonzero(filled == 0))


@pytest.mark.parametrize("bt", [0, 1, 2])
def test_ties(edges, bt):
    """every family is there; an input with ties on the survivor path is one on which the ties-high decoder returns other bits"""
    groups, _, model = edges
    seen = {}
    for (name, x, bits, _, _), r in zip(groups[(bt, N)], model[(bt, N)]):
        if name.startswith("tie:"):
            seen[name] = r
            assert r.total["tie"] > 0
            if r.on_path["tie"]:
                assert not np.array_equal(r.bits_ties_high, bits), name
    assert sorted(seen) == sorted(TIES)
    assert seen["tie:all-0.5"].on_path["tie"] == N - V.ORDER and not seen["tie:all-0.5"].bits.any()
    for name in ("tie:flat 1e-6", "tie:flat 3e-7"):
        assert seen[name].on_path["tie"] >= 50, (name, seen[name].on_path)


@pytest.mark.parametrize("bt", [0, 1, 2])
def test_magnitudes_nan_and_inf(edges, bt):
    """the families are there, and the stored values are the reference's answers to them: a NaN before the last step kills the
    trellis (every metric fails old >= 0 one step later: error -1 / length), one in the last step is the error value itself,
    and costs that overflow end at +inf"""
    groups, _, _ = edges
    R = V.rate(bt)
    by_name = {name: (x, bits, err) for name, x, bits, err, _ in groups[(bt, N)]}
    assert set(MAGNITUDES + NAN_INF) <= set(by_name)
    dead = np.float32(-1) / np.float32(N * R)
    for name, where in (("nan:index 0 only", [0]), ("nan:index 1", [1]), ("nan:step 20", [20 * R + 1])):
        x, bits, err = by_name[name]
        assert np.flatnonzero(np.isnan(x)).tolist() == where and V.same_float(err, dead) and not bits[21:].any(), name
    x, bits, err = by_name["nan:last step"]
    assert np.flatnonzero(np.isnan(x)).tolist() == [(N - 1) * R + 2] and np.isnan(err)
    for name, n_inf in (("inf:single +inf", 1), ("inf:+inf and -inf in one step", 2)):
        x, bits, err = by_name[name]
        assert np.count_nonzero(np.isinf(x)) == n_inf and not np.isnan(x).any() and err == np.inf, name
    for name in ("mag:+-1e+19", "mag:+-3e+38"):
        assert np.isfinite(by_name[name][0]).all() and by_name[name][2] == np.inf, name
    x = by_name["mag:-0.0 and denormals"][0]
    tiny = np.abs(x) < np.finfo(np.float32).tiny
    assert np.count_nonzero(tiny & (x != 0)) > 50 and np.count_nonzero(np.signbit(x) & (x == 0)) > 50
    assert 5e3 < by_name["mag:offset 100"][2] < 2e4                # ~ 1e4 per code bit: the last metrics are ~ 1e7, their ulp is 1


def test_other_lengths(edges):
    groups, _, _ = edges
    for bt in (0, 2):
        for n in V.LENGTHS:
            assert sorted(i[0] for i in groups[(bt, n)]) == ["len:flat 1e-6", "len:gaussian 0.7"]


def test_gaussian_inputs_do_not_tell_the_wrong_decoders_apart():
    """The gap this material closes: on the inputs of test_gpu_parity.py::test_viterbi_bit_exact and of the decodes that
    test_viterbi_one_launch_equals_the_launch_chain compares with the oracle (0 / 1 codewords with Gaussian noise), a decoder
    without the repeat path and one that hands ties to the high predecessor both return the reference's bits: no merged
    decision and no tie lies on a survivor path there."""
    inputs = []
    for bt in (0, 1, 2):
        rng = np.random.default_rng(200 + bt)
        for sigma in (0.0, 0.3, 0.5, 0.7, 1.5):
            coded = orc.conv_encode(bt, rng.integers(0, 2, 128)).astype(np.float32)
            inputs.append((bt, (coded + rng.normal(0, sigma, coded.shape)).astype(np.float32)))
    rng = np.random.default_rng(77)
    for bt in (0, 1, 2):
        bits = rng.integers(0, 2, (3, 128))
        coded = np.stack([orc.conv_encode(bt, b) for b in bits]).astype(np.float32)
        inputs += [(bt, s) for s in (coded + rng.normal(0, 0.5, coded.shape)).astype(np.float32)]
    assert len(inputs) == 24
    for bt, x in inputs:
        r = V.decode(bt, x)
        pinned(bt, x, r)
        # (sigma 0 is hard 0 / 1 input: ties exist, the survivor costs 0 and meets none)
        assert r.on_path["merged"] == 0 and r.on_path["tie"] == 0
        assert np.array_equal(r.bits_merge_blind, r.bits) and np.array_equal(r.bits_ties_high, r.bits)
