#!/usr/bin/env python3
"""Writes tests/golden/viterbi_edges.npz: the inputs on which K8 (csrc/hip/viterbi.hip) is held to conv_decode_soft beyond a plain
add-compare-select -- merged chains steered onto the survivor path, exact ties, extreme magnitudes, NaN and inf away from the
first position, and trellis lengths other than 143.  Seeded, CPU only: it needs the oracle (oracle/libawm_oracle.so) and
tests/_viterbi.py, nothing else, and a rerun reproduces the file byte for byte (the archive is written with fixed time stamps).

    python tests/golden/make_viterbi_edges.py          (about two minutes)

Per group (code type A / B / AB, trellis length n):  <TYPE><n>_in [k][n * rate] float32, _bits [k][n - 15] int8 and _err [k]
float32 as the oracle returns them, _name [k] the family of each input, _tm [k][2] the steered decision (step, state) or -1.
empty_cells names the (type, cell) pairs for which no steered input was found within the budget.

What is kept and why is decided by the model in tests/_viterbi.py; tests/test_viterbi_restated.py re-checks every condition on
the stored file."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _oracle as orc  # noqa: E402
import _viterbi as V  # noqa: E402

OUT = os.path.join(HERE, "viterbi_edges.npz")
TYPES = V.TYPES
N = 143
LENGTHS = V.LENGTHS
# the steps at which a steered merge is looked for: two or three per cell of _viterbi.CELLS
TARGETS = (15, 15, 24, 61, 110, 28, 77, 116, 35, 58, 130, 132, 133, 134, 135)
SCALES = (1e-5, 3e-5, 3e-6, 1e-4)


class Groups:
    def __init__(self):
        self.g = {}

    def add(self, bt, name, x, tm=(-1, -1)):
        x = np.ascontiguousarray(x, np.float32)
        bits, err = orc.conv_decode_soft(bt, x)
        r = V.decode(bt, x, classes=False)
        assert np.array_equal(bits, r.bits) and (np.float32(err).tobytes() == r.error.tobytes() or (np.isnan(err) and np.isnan(r.error))), name
        self.g.setdefault((bt, x.size // V.rate(bt)), []).append((name, x, bits.astype(np.int8), np.float32(err), tm))

    def arrays(self):
        out = {}
        for (bt, n), items in sorted(self.g.items()):
            k = "%s%d" % (TYPES[bt], n)
            out[k + "_in"] = np.stack([i[1] for i in items])
            out[k + "_bits"] = np.stack([i[2] for i in items]).reshape(len(items), max(0, n - V.ORDER))
            out[k + "_err"] = np.array([i[3] for i in items], np.float32)
            out[k + "_name"] = np.array([i[0] for i in items], "U40")
            out[k + "_tm"] = np.array([i[4] for i in items], np.int32)
        return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def steered(groups, bt):
    """One input per target step where the model confirms it: a merged decision on the survivor path that the merge-blind
    decoder gets wrong.  The prefix is V.flat_level: chains merge where the metrics cross a power of two, so the step-0 offset
    puts that crossing into the wanted step."""
    filled = np.zeros(len(V.CELLS), int)
    for ti, target in enumerate(TARGETS):
        done = False
        for attempt, s in enumerate(SCALES * 3):
            rng = np.random.default_rng([8, bt, ti, attempt])
            prefix = V.flat_level(bt, rng, N, s, target)
            r = V.decode(bt, prefix)
            st, ms = np.nonzero(r.cls == V.MERGED)
            cand = [(int(t), int(m)) for t, m in zip(st, ms) if V.cell_of(t) == V.cell_of(target) and V.steerable(t, m, N)]
            for pick in rng.permutation(len(cand))[:3]:
                t, m = cand[pick]
                x = V.steer(bt, rng, prefix, t, m)
                q = V.decode(bt, x)
                # (m and m ^ 0x4000 have the same successors, hence the same clean tail: the survivor takes the better of the two)
                m = int(q.path[t])
                if q.cls[t, m] == V.MERGED and not np.array_equal(q.bits, q.bits_merge_blind):
                    groups.add(bt, "steered", x, (t, m))
                    filled[V.cell_of(t)] += 1
                    print("  %-2s steered target %3d -> step %3d state %5d (s = %g): on the path %s" % (TYPES[bt], target, t, m, s, q.on_path), flush=True)
                    done = True
                    break
            if done:
                break
        if not done:
            print("  %-2s steered target %3d: nothing confirmed within the budget" % (TYPES[bt], target), flush=True)
    return filled


def hard(bt, rng, flips):
    bits = np.concatenate([rng.integers(0, 2, N - V.ORDER), np.zeros(V.ORDER, np.int64)])
    cw, _ = V.encode(bt, bits)
    return np.where(rng.random(cw.size) < flips, 1 - cw, cw).astype(np.float32)


def tie_families(bt):
    def erased(rng):
        x = hard(bt, rng, 0.0)
        x[rng.random(x.size) < 0.5] = 0.5
        return x
    return (("tie:all-0.5", lambda rng: np.full(N * V.rate(bt), 0.5, np.float32)),
            ("tie:hard, 10% flipped", lambda rng: hard(bt, rng, 0.10)),
            ("tie:hard, 30% flipped", lambda rng: hard(bt, rng, 0.30)),
            ("tie:quarters", lambda rng: (np.round(V.gaussian(bt, rng, N, 0.5) * 4) / 4).astype(np.float32)),
            ("tie:half erased", erased),
            ("tie:flat 1e-6", lambda rng: V.flat(bt, rng, N, 0.5, 1e-6)),
            ("tie:flat 3e-7", lambda rng: V.flat(bt, rng, N, 0.5, 3e-7)))


def ties(groups, bt):
    """Per family the first input with ties ON the survivor path for which the ties-high decoder returns other bits.  A family
    that puts none there within its budget (lightly flipped hard bits: the survivor wins clearly) is kept for its ties off the
    path; an input with ties on the path that ties-high survives is never kept."""
    for fi, (name, make) in enumerate(tie_families(bt)):
        spare = None
        for attempt in range(8):
            x = make(np.random.default_rng([9, bt, fi, attempt]))
            r = V.decode(bt, x)
            if r.on_path["tie"] >= 1 and not np.array_equal(r.bits, r.bits_ties_high):
                spare = (x, r)
                break
            if r.on_path["tie"] == 0 and spare is None:
                spare = (x, r)
        x, r = spare
        groups.add(bt, name, x)
        print("  %-2s %-22s on the path %s, of %s" % (TYPES[bt], name, r.on_path, r.total), flush=True)


def magnitudes(groups, bt):
    rng = np.random.default_rng([10, bt])
    groups.add(bt, "mag:offset 100", V.gaussian(bt, rng, N, 0.5) + np.float32(100))
    groups.add(bt, "mag:1e-3 about 0.5", (V.gaussian(bt, rng, N, 0.5).astype(np.float64) * 1e-3 + 0.5).astype(np.float32))
    for big in (1e19, 3e38):
        groups.add(bt, "mag:+-%g" % big, ((2 * hard(bt, rng, 0.1) - 1) * np.float32(big)).astype(np.float32))
    x = hard(bt, rng, 0.1)
    small = rng.choice(np.array([-0.0, 1e-40, -1e-40, 1.4e-45, 0.0], np.float32), x.size)
    groups.add(bt, "mag:-0.0 and denormals", np.where(x == 0, small, x).astype(np.float32))


def nan_inf(groups, bt):
    R = V.rate(bt)
    rng = np.random.default_rng([11, bt])
    for name, pokes in (("nan:index 0 only", [(0, np.nan)]), ("nan:index 1", [(1, np.nan)]), ("nan:last step", [((N - 1) * R + 2, np.nan)]),
                        ("nan:step 20", [(20 * R + 1, np.nan)]), ("inf:single +inf", [(30 * R + 3, np.inf)]),
                        ("inf:+inf and -inf in one step", [(40 * R, np.inf), (40 * R + 3, -np.inf)])):
        x = V.gaussian(bt, rng, N, 0.5)
        for i, v in pokes:
            x[i] = v
        groups.add(bt, name, x)


def lengths(groups, bt):
    for n in LENGTHS:
        rng = np.random.default_rng([12, bt, n])
        groups.add(bt, "len:gaussian 0.7", V.gaussian(bt, rng, n, 0.7))
        groups.add(bt, "len:flat 1e-6", V.flat(bt, rng, n, 0.5, 1e-6))


def main():
    groups = Groups()
    empty = []
    for bt in (0, 1, 2):
        filled = steered(groups, bt)
        print("%-2s cells filled: %s" % (TYPES[bt], dict(zip(V.CELLS, filled.tolist()))), flush=True)
        for c in np.flatnonzero(filled == 0):
            print("%-2s EMPTY CELL: %s" % (TYPES[bt], V.CELLS[c]))
            empty.append("%s: %s" % (TYPES[bt], V.CELLS[c]))
        assert filled.sum() >= 6 and np.count_nonzero(filled == 0) <= 1, "too few steered inputs"
        ties(groups, bt)
        magnitudes(groups, bt)
        nan_inf(groups, bt)
        if bt != 1:
            lengths(groups, bt)
    arrays = groups.arrays()
    arrays["empty_cells"] = np.array(empty, "U60")
    write_npz(OUT, arrays)
    print("written: %s, %d bytes, %d inputs in %d groups" % (os.path.relpath(OUT), os.path.getsize(OUT),
                                                           sum(len(v) for v in groups.g.values()), len(groups.g)))


if __name__ == "__main__":
    main()
