"""The approximate sync search restated in numpy, and the shapes that sit on the edges of the streaming scan kernel (K5w).
TEST INFRASTRUCTURE ONLY; plain numpy, no GPU.

scan() restates SyncFinder::bit_quality / sync_decode (reference syncfinder.cc:94-153) for every start frame at once and
local_mean() the local mean of search_approx (syncfinder.cc:234-254); silent_range() is scan_silence (syncfinder.cc:155-169).
The restatement is vectorised over the START FRAMES only: every candidate still runs the reference's loops in the reference's
order (bit, sync frame, 30 x "up then down"), each float32 addition rounded on its own -- the shape in which it equals the oracle
and the compiled reference to the last bit (test_scan_restated.py pins that before test_gpu_scan_edges.py leans on it).

The shapes: K5w works in tiles of 252 candidates (a wave of 64 lanes x 4 candidates that drops its last lane), its tiles are dealt
to 8 XCDs in ranges of ceil (tiles / 8), it reads the dB matrix in chunks of 64 frames with a padded leading dimension, and in
clip mode it follows the one run of frames that were transformed.  BLOCK and CLIP below put a candidate count, a matrix end or
an end of that run on each of these borders."""
import numpy as np

import _oracle as orc

PAY = "0123456789abcdef0011223344556677"
FRAME = 1024
SHIFTS = 4                              # Params::frame_size / Params::sync_search_step
STEP = FRAME // SHIFTS
BLOCK_FRAMES = 2226                     # mark_sync_frame_count() + mark_data_frame_count()
CLIP_BUFFER_FRAMES = 3 * (BLOCK_FRAMES + 5)
LOCAL_MEAN_DISTANCE = 20                # syncfinder.hh:88


def total_frames(clip):
    return 2 * BLOCK_FRAMES if clip else BLOCK_FRAMES


def counts(n_frames, clip):
    """(n_db, S): dB rows per shift (sync_fft_parallel drops the last frame, syncfinder.cc:632) and start frames with
    (start + total) * 81 < db.size() (syncfinder.cc:189-193)"""
    n_db = n_frames // FRAME - 1
    return n_db, n_db - total_frames(clip)


def silent_range(pcm, clip):
    """(first, last) in VALUES (frames x channels): scan_silence in clip mode, everything in block mode (syncfinder.cc:494-503)"""
    v = np.asarray(pcm).ravel()
    if not clip:
        return 0, v.size
    nz = np.flatnonzero(v)
    if nz.size == 0:
        return v.size, v.size
    return int(nz[0]), int(nz[-1]) + 1


def scan(tab, db, have, S, water_delta=0.01):
    """sync_decode (tab, s, db, have) for s < S.  tab: orc.sync_bits [6][rows][frame, 30 up, 30 down];
    db [n_db][81] float32 and have [n_db] as sync_fft returns them"""
    tab = np.asarray(tab)
    dbt = np.ascontiguousarray(np.asarray(db, np.float32).T)                  # [band][frame]: a term of all candidates is one slice
    have = np.asarray(have) != 0
    assert dbt.dtype == np.float32 and int(tab[:, :, 0].max()) + S <= dbt.shape[1] == have.size
    q = np.zeros(S, np.float64)
    total = np.zeros(S, np.int64)
    for bit in range(tab.shape[0]):
        um = np.zeros(S, np.float32)
        dm = np.zeros(S, np.float32)
        n = np.zeros(S, np.int64)
        for row in tab[bit]:
            f = int(row[0])
            h = have[f:f + S]
            if not h.any():
                continue
            u, d = um.copy(), dm.copy()
            for i in range(30):
                u += dbt[row[1 + i], f:f + S]
                d += dbt[row[31 + i], f:f + S]
            um = np.where(h, u, um)                                           # (a candidate whose frame was skipped keeps its sums)
            dm = np.where(h, d, dm)
            n += h
        assert um.dtype == np.float32 and dm.dtype == np.float32
        # bit_quality: float division and subtraction, then double
        with np.errstate(divide="ignore", invalid="ignore"):
            raw = np.where((um == 0) | (dm == 0), np.float32(0),
                           np.where(um < dm, np.float32(1) - um / dm, dm / um - np.float32(1)))
        assert raw.dtype == np.float32
        raw = raw.astype(np.float64)
        q += (raw if bit & 1 else -raw) * n
        total += n
    q = np.where(total != 0, q / np.maximum(total, 1), q)
    return q / min(water_delta, 0.080) / 2.9                                  # normalize_sync_quality


def local_mean(raw):
    """the mean of the 41 neighbours without the 7 in the middle, added in ascending order, over the scores sorted by index"""
    raw = np.asarray(raw, np.float64)
    n_scores = raw.size
    avg = np.zeros(n_scores, np.float64)
    n = np.zeros(n_scores, np.int64)
    i = np.arange(n_scores)
    for j in range(-LOCAL_MEAN_DISTANCE, LOCAL_MEAN_DISTANCE + 1):
        if abs(j) >= 4:
            ok = (i + j >= 0) & (i + j < n_scores)
            avg[ok] += raw[i[ok] + j]
            n += ok
    return np.where(n > 0, avg / np.maximum(n, 1), avg)


def search_approx(tab, planes, S):
    """(index, raw_quality, local_mean) of SyncFinder::search_approx from the (db, have) of the four shifts"""
    assert len(planes) == SHIFTS
    raw = np.zeros((S, SHIFTS), np.float64)
    for shift, (db, have) in enumerate(planes):
        raw[:, shift] = scan(tab, db, have, S)
    raw = raw.ravel()
    index = (np.arange(S, dtype=np.uint64)[:, None] * FRAME + np.arange(SHIFTS, dtype=np.uint64) * STEP).ravel()
    return index, raw, local_mean(raw)


def planes_of(sync_fft, pcm, clip):
    """the four (db, have) of search_approx through sync_fft (index, frame_count, want_frames, first, last) of the caller"""
    n_db, _ = counts(pcm.shape[0], clip)
    first, last = silent_range(pcm, clip)
    return [sync_fft(shift * STEP, n_db, None, first, last) for shift in range(SHIFTS)]


# ---- material --------------------------------------------------------------------------------------------------------------------
def noise(seed, n, ch):
    return np.random.default_rng(seed).uniform(-1, 1, (n, ch)).astype(np.float32)


def marked(seed, n, ch, key=None):
    return orc.add(key, noise(seed, n, ch), ch, PAY).reshape(n, ch)


def clip_padded(x):
    """a clip as ClipDecoder pads it: always CLIP_BUFFER_FRAMES long, the clip ends one padded block before the buffer does"""
    ch = x.shape[1]
    n = (BLOCK_FRAMES + 5) * FRAME * ch
    vals = x.ravel()
    last = min(n, vals.size)
    pad_start = n + (n - last if last < n else 0)
    return np.concatenate([np.zeros(pad_start, np.float32), vals[:last], np.zeros(n, np.float32)]).reshape(-1, ch)


# block mode: (S, channels, extra samples, test key 42).  n = (2226 + 1 + S) * 1024 + extra
BLOCK = [
    (1, 2, 0, False),            # one candidate, one tile; 7 of the 8 XCD slots return at once
    (3, 1, 300, False), (4, 3, 1023, False), (5, 2, 300, False),               # the quad of a lane
    (251, 3, 0, False), (252, 1, 1023, False), (253, 2, 300, False),           # the tile
    (505, 2, 0, False),          # 2 x 252 + 1
    (2017, 1, 300, False),       # 8 x 252 + 1: two tiles per XCD, most slots return.  (The largest rows have the fewest channels:
                                 # on the CPU a case costs orc.add + four sync_fft + a search per side, all linear in the channels)
    (14, 2, 1023, False), (15, 3, 0, False), (78, 1, 300, False),              # n_db = 2240, 2241, 2304: the padded leading
                                 # dimension is n_db itself or just past it, the loader's substitute for frames past the matrix is live
    (253, 2, 300, True), (15, 3, 0, True),         # two of the rows under another key
]

# clip mode: the buffer is CLIP_BUFFER_FRAMES = 6693 frames long, S = 2240 = 9 tiles.
# ("padded", clip length in samples, channels, samples zeroed at the start, at the end) goes through clip_padded;
# ("placed", frame offset, channels, shift in samples) puts a clip of 300 frames into an all-zero buffer by hand.
#
# The placed offsets: a candidate s sees the clip only if s < offset + 300 and s + 4452 > offset, so the offsets 0, 251, 252 and
# 6392 leave at most 300, 551, 552 and 300 of the 2240 candidates of a shift with anything to add: such a case would pass all but
# empty.  In their place stand 960, 1259, 1260 and 5376, where 1120 candidates and more are live and the run [offset, offset + 300)
# keeps the same relation to the borders: 960 = 15 x 64 starts ON a chunk border and ends on 1260 = 5 x 252, a tile's first
# candidate; 1259 starts one frame before that candidate and 1260 on it; 5376 = 84 x 64 lies behind every first candidate, so that
# only the sync frames of the second block are live.  2226 (inside tile 8; the run ends in tile 10) and 4152 (the run ends on 4452,
# the last frame candidate 0 can see) stand as they were.  The shift by 517 samples moves both ends into a frame.
# What the replaced offsets would have held and these do not: a run that starts at frame 0 or ends at the buffer's last frame, where
# K5w's chunk range is c_lo = 0 or c_hi = n_chunks.  Only the padded clips come near that: the 2231-frame one ends 2231 frames before
# the buffer does, and no run here starts before frame 960.
PLACED_FRAMES = 300
CLIP = ([("padded", 3 * 1024, 2, 0, 0), ("padded", 64 * 1024, 1, 0, 0), ("padded", 255 * 1024 + 1023, 3, 0, 0),
         ("padded", 257 * 1024 + 5, 2, 0, 0), ("padded", 900 * 1024 + 77, 3, 0, 0), ("padded", 2231 * 1024, 1, 0, 0),
         ("padded", 900 * 1024 + 77, 2, 1500, 0), ("padded", 700 * 1024 + 77, 3, 0, 700)]
        + [("placed", off, 1 + k % 3, shift) for k, off in enumerate((960, 1259, 1260, 2226, 4152, 5376)) for shift in (0, 517)])


def block_id(c):
    return "S%d-ch%d-x%d%s" % (c[0], c[1], c[2], "-key42" if c[3] else "")


def clip_id(c):
    if c[0] == "padded":
        return "padded%d-ch%d%s%s" % (c[1], c[2], "-head%d" % c[3] if c[3] else "", "-tail%d" % c[4] if c[4] else "")
    return "placed%d-ch%d+%d" % (c[1], c[2], c[3])


def block_pcm(case, key42):
    S, ch, extra, use_key = case
    n = (BLOCK_FRAMES + 1 + S) * FRAME + extra
    pcm = marked(1000 + S + ch, n, ch, key42 if use_key else None)
    assert counts(n, False) == (BLOCK_FRAMES + S, S)
    return (key42 if use_key else None), pcm


def clip_pcm(case):
    if case[0] == "padded":
        _, n, ch, head, tail = case
        x = marked(2000 + n % 1009 + ch, n, ch)
        x[:head] = 0
        if tail:
            x[-tail:] = 0
        pcm = clip_padded(x)
    else:
        _, off, ch, shift = case
        x = marked(3000 + off + ch, PLACED_FRAMES * FRAME, ch)
        pcm = np.zeros((CLIP_BUFFER_FRAMES * FRAME, ch), np.float32)
        pcm[off * FRAME + shift:off * FRAME + shift + len(x)] = x
    assert counts(len(pcm), True) == (CLIP_BUFFER_FRAMES - 1, 2240)
    return pcm
