"""conv_decode_soft restated in numpy with a view of every decision, two deliberately wrong decoders, and a builder of inputs
that put the rare decisions of the HIP decoder (K8, csrc/hip/viterbi.hip) on the survivor path.
TEST INFRASTRUCTURE ONLY; plain numpy, no GPU.

decode() restates the reference's loop (convcode.cc:128-213) for all 32768 successor states at once: one float32 array of
metrics, the two predecessors ns >> 1 and (ns >> 1) | 0x4000 of every successor, delta += (cbit - sbit)^2 term by term in
float32 and in generator order, the reference's select (old >= 0 reachability; delta < new || new < 0 with the low predecessor
visited first), the walk back from state 0 and error = metric[0] / float32 (coded length).  test_viterbi_restated.py pins it to
the oracle bit for bit before anything leans on it.

K8 replaces the two chains of additions per successor by one (the chain of the smaller predecessor) and decides "high
predecessor wins" as old1 < old0; a wave repeats a step with both chains when a lane sees  !(hi - lo > 2^-19 (hi + sum_max)).
So every decision with both predecessors reachable gets a class here:
    TIE     old1 == old0                                   the low predecessor keeps it (strict "<")
    MERGED  old1 <  old0 but the two sums end equal        the low predecessor keeps it; what the kernel's repeat path exists for
    NEAR    old1 <  old0 inside the kernel's window, the sums still differ (the repeat path runs and changes nothing)
The three decoders share their metrics (a tie or a merge leaves the sum the same whoever wins) and differ in decisions only, so
one pass yields all of them:
    bits              the reference
    bits_merge_blind  decision old1 < old0 wherever both predecessors are reachable (a kernel without the repeat path)
    bits_ties_high    decision d1 <= d0 (ties handed to the high predecessor)"""
import numpy as np

ORDER = 15
STATES = 1 << ORDER
GEN_AB = (0o66561, 0o75211, 0o71545, 0o54435, 0o63635, 0o52475, 0o63543, 0o75307, 0o52547, 0o45627, 0o67657, 0o51757)
TIE, MERGED, NEAR = 1, 2, 3
WINDOW = np.float32(2.0 ** -19)

_NS = np.arange(STATES, dtype=np.int64)
_P0 = _NS >> 1
_P1 = _P0 | (STATES >> 1)
_sbits = {}


def generators(bt):
    return GEN_AB if bt == 2 else GEN_AB[bt::2]


def rate(bt):
    return 12 if bt == 2 else 6


def _parity(v):
    v = v ^ (v >> 16)
    v = v ^ (v >> 8)
    v = v ^ (v >> 4)
    v = v ^ (v >> 2)
    v = v ^ (v >> 1)
    return (v & 1).astype(bool)


def sbits(bt):
    """[rate][state]: the code bits a transition INTO the state emits"""
    if bt not in _sbits:
        _sbits[bt] = np.stack([_parity(_NS & g) for g in generators(bt)])
    return _sbits[bt]


def encode(bt, bits, state=0):
    """conv_encode's code bits for the input bits, from the given register state on (no termination added)"""
    out = np.zeros((len(bits), rate(bt)), np.int32)
    gens = generators(bt)
    for i, b in enumerate(bits):
        state = ((state << 1) | int(b)) & (STATES - 1)
        out[i] = [bin(state & g).count("1") & 1 for g in gens]
    return out.ravel(), state


class Result:
    pass


def decode(bt, coded, classes=True):
    coded = np.ascontiguousarray(coded, np.float32)
    R = rate(bt)
    assert coded.ndim == 1 and coded.size % R == 0 and coded.size >= R
    n_steps = coded.size // R
    sb = sbits(bt)
    metric = np.full(STATES, -1, np.float32)
    metric[0] = 0
    dec = np.zeros((3, n_steps, STATES), bool)                     # reference, merge-blind, ties-high
    cls = np.zeros((n_steps, STATES), np.uint8)
    one = np.float32(1)
    with np.errstate(all="ignore"):
        for step in range(n_steps):
            c = coded[step * R:(step + 1) * R]
            e0 = c * c
            e1 = (c - one) * (c - one)
            old0, old1 = metric[_P0], metric[_P1]
            d0, d1 = old0.copy(), old1.copy()
            for p in range(R):
                term = np.where(sb[p], e1[p], e0[p])
                d0 += term
                d1 += term
            r0, r1 = old0 >= 0, old1 >= 0
            both = r0 & r1
            dec[0, step] = r1 & (~r0 | (d1 < d0))
            dec[1, step] = r1 & (~r0 | (old1 < old0))
            dec[2, step] = r1 & (~r0 | (d1 <= d0))
            metric = np.where(dec[0, step], d1, np.where(r0, d0, np.float32(-1))).astype(np.float32)
            if classes:
                sum_max = np.float32(0)
                for p in range(R):
                    sum_max = np.float32(sum_max + max(e0[p], e1[p]))
                high = both & (old1 < old0)
                window = high & ~((old0 - old1) > WINDOW * (old0 + sum_max))
                k = cls[step]
                k[both & (old1 == old0)] = TIE
                k[window & (d1 < d0)] = NEAR
                k[high & (d1 == d0)] = MERGED
        res = Result()
        res.error = np.float32(metric[0] / np.float32(coded.size))
    res.n_steps = n_steps
    n_out = max(0, n_steps - ORDER)
    paths = []
    for v in range(3):
        state, bits, path = 0, np.zeros(n_steps, np.int32), np.zeros(n_steps, np.int64)
        for step in range(n_steps - 1, -1, -1):
            path[step] = state
            bits[step] = state & 1
            state = (state >> 1) | (int(dec[v, step, state]) << (ORDER - 1))
        paths.append((bits[:n_out], path))
    res.bits, res.path = paths[0]
    res.bits_merge_blind, res.bits_ties_high = paths[1][0], paths[2][0]
    res.cls = cls if classes else None
    on_path = cls[np.arange(n_steps), res.path]
    res.total = {name: int(np.count_nonzero(cls == v)) for name, v in (("tie", TIE), ("merged", MERGED), ("near", NEAR))}
    res.on_path = {name: int(np.count_nonzero(on_path == v)) for name, v in (("tie", TIE), ("merged", MERGED), ("near", NEAR))}
    res.path_steps = {name: np.flatnonzero(on_path == v) for name, v in (("tie", TIE), ("merged", MERGED), ("near", NEAR))}
    return res


# ---- input families ------------------------------------------------------------------------------------------------
def flat(bt, rng, n_steps, centre, s):
    """a codeword squeezed to centre -/+ s with noise of the same size: all path metrics stay within a few ulp of each other"""
    bits = np.concatenate([rng.integers(0, 2, max(0, n_steps - ORDER)), np.zeros(min(ORDER, n_steps), np.int64)])
    cw, _ = encode(bt, bits)
    return (centre + (cw - 0.5) * 2 * s + rng.normal(0, s, cw.size)).astype(np.float32)


def flat_level(bt, rng, n_steps, s, t):
    """flat (centre 0.5) with the metrics of ALL paths lifted so that they cross a power of two during step t.  Two chains that
    start one ulp apart stay one ulp apart while they share a binade; they can merge only where the ulp doubles, so merged
    decisions sit in the steps where the metrics cross a power of two -- with 0.25 per code bit that is wherever 0.25 * rate *
    step happens to cross one.  Step 0 moves that: the code bits of its two branches are all 0 or all 1 (every generator is odd),
    so soft bits 0.5 + a, 0.5 - a in turns cost rate * (0.25 + a^2) on either branch -- exactly, as a is a multiple of 1 / 32."""
    R = rate(bt)
    assert t >= 1 and R % 2 == 0
    k = 0
    while 2.0 ** k / R - 0.125 - 0.25 * t < 0.02:
        k += 1
    a = np.round(np.sqrt(2.0 ** k / R - 0.125 - 0.25 * t) * 32) / 32
    x = flat(bt, rng, n_steps, 0.5, s)
    x[:R] = 0.5 + a * np.where(np.arange(R) % 2 == 0, 1, -1)
    return x


def gaussian(bt, rng, n_steps, sigma):
    bits = np.concatenate([rng.integers(0, 2, max(0, n_steps - ORDER)), np.zeros(min(ORDER, n_steps), np.int64)])
    cw, _ = encode(bt, bits)
    return (cw + rng.normal(0, sigma, cw.size)).astype(np.float32)


def steerable(t, m, n_steps):
    """can a path that is in state m after step t still end in state 0 (the remaining steps are all termination zeros)?"""
    left = n_steps - 1 - t
    return left >= ORDER or (m & ((1 << (ORDER - left)) - 1)) == 0


def steer(bt, rng, prefix, t, m):
    """the prefix up to and including step t, then a clean 0 / 1 codeword that leaves state m and ends in state 0: that path
    costs nothing more and every other one at least 1 -- except the one through m ^ 0x4000, which has the same successors and the
    same tail: the survivor runs through the decision (t, m) or through (t, m ^ 0x4000), whichever metric is smaller"""
    R = rate(bt)
    n_steps = prefix.size // R
    assert steerable(t, m, n_steps)
    left = n_steps - 1 - t
    bits = np.concatenate([rng.integers(0, 2, max(0, left - ORDER)), np.zeros(min(ORDER, left), np.int64)])
    cw, end = encode(bt, bits, m)
    assert end == 0
    return np.concatenate([prefix[:(t + 1) * R], cw.astype(np.float32)])


TYPES = ("A", "B", "AB")
# trellis lengths besides the product's 143: every residue mod 4, no payload bits (15), plans whose rounds are all checked (15 - 17),
# a last round of 4 or of 3 that is not plain, only 12-step launches (144), the largest plan (256 = 64 rounds)
LENGTHS = (15, 16, 17, 18, 19, 20, 21, 22, 23, 27, 144, 145, 146, 256)


def load_edges(path):
    """tests/golden/viterbi_edges.npz as {(bt, n_steps): [(name, soft, bits, error, (t, m))]} and the list of empty cells"""
    z = np.load(path)
    groups = {}
    for key in z.files:
        if key.endswith("_in"):
            k = key[:-3]
            bt = 2 if k.startswith("AB") else TYPES.index(k[0])
            n = int(k[len(TYPES[bt]):])
            groups[(bt, n)] = [(str(z[k + "_name"][i]), z[k + "_in"][i], z[k + "_bits"][i].astype(np.int32), z[k + "_err"][i],
                                tuple(int(v) for v in z[k + "_tm"][i])) for i in range(len(z[key]))]
    return groups, [str(c) for c in z["empty_cells"]]


def same_float(a, b):
    """equal as float32 bit patterns, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


CELLS = ("step<=15", "12-step launch, steps 0-3", "12-step launch, steps 4-7", "12-step launch, steps 8-11", "steps 132-139")


def cell_of(t):
    """where step t of a 143-step decode runs in K8: the checked rounds, a third of a 12-step launch, the single 4-step rounds"""
    if t <= 15:
        return 0
    if t <= 131:
        return 1 + (t % 12) // 4
    return 4 if t <= 139 else None
