"""The limiter restated in numpy, and material on which a wrong limiter shows.  TEST INFRASTRUCTURE ONLY; plain numpy, no GPU.

np_limiter restates Limiter::block_max / process_block / flush (reference limiter.cc:90-153) in float32 with every operation
rounded on its own -- the shape in which it equals the oracle and the compiled reference to the last bit
(test_limiter_restated.py pins that before test_gpu_limiter.py leans on it).

The materials sit on a floor of uniform noise at +-0.05, far under the ceiling of 0.99, and carry a few loud samples in chosen
places: the ramps between neighbouring blocks are then steep (1e-5 per sample instead of the 1e-9 of full-scale noise) and the
block maxima sit ON block boundaries, where a sample counted in the wrong block changes a maximum."""
import numpy as np

CEILING = np.float32(0.99)          # Limiter::set_ceiling (reference wmadd.cc)
FLOOR = 0.05


def _frames(a):
    a = np.asarray(a, np.float32)
    return a.reshape(a.shape[0], -1)


def block_maxima(mix, block_size, ceiling=CEILING, grid_shift=0):
    """max (ceiling, max |mix| over block b) for b < ceil (n / block_size)   (Limiter::block_max)
    grid_shift: the WRONG grid of the mutants in test_limiter_restated.py -- block b covers the samples
    [b BS + grid_shift, (b + 1) BS + grid_shift); samples that fall off either end count in the first / last block"""
    x = _frames(mix)
    n = x.shape[0]
    n_blocks = -(-n // block_size)
    out = np.full(n_blocks, ceiling, np.float32)
    if n:
        b = np.clip((np.arange(n, dtype=np.int64) - grid_shift) // block_size, 0, n_blocks - 1)
        np.maximum.at(out, b, np.abs(x).max(axis=1))
    return out


def ramp(data, first_sample, block_max, block_size, first_block=0, ceiling=CEILING, index_offset=0):
    """Limiter::process_block on `data`, whose first frame is sample first_sample of the stream, with GIVEN block maxima:
    block_max[k] belongs to block first_block + k; entries under the ceiling count as the ceiling, and so does every block
    outside the table (block_max_last starts at the ceiling, flush() appends silence).
    index_offset: the WRONG ramp index i + index_offset of the mutant in test_limiter_restated.py"""
    x = np.asarray(data, np.float32)
    n = x.shape[0]
    if n == 0:
        return x.copy()
    ceiling = np.float32(ceiling)
    bm = np.asarray(block_max, np.float32)
    gs = first_sample + np.arange(n, dtype=np.int64)
    b = gs // block_size
    i = (gs - b * block_size + index_offset).astype(np.float32)
    blocks = np.arange(b[0] - 1, b[-1] + 2, dtype=np.int64)          # every block the ramps of b[0] .. b[-1] look at
    k = blocks - first_block
    inside = (blocks >= 0) & (k >= 0) & (k < len(bm))
    m = np.full(len(blocks), ceiling, np.float32)
    m[inside] = np.maximum(bm[k[inside]], ceiling)
    m_last, m_cur, m_next = m[:-2], m[1:-1], m[2:]
    scale_start = ceiling / np.maximum(m_last, m_cur)
    scale_end = ceiling / np.maximum(m_cur, m_next)
    scale_step = (scale_end - scale_start) / np.float32(block_size)
    j = b - b[0]
    scale = scale_start[j] + i * scale_step[j]
    assert scale.dtype == np.float32
    return x * (scale if x.ndim == 1 else scale[:, None])


def np_limiter(mix, block_size, ceiling=np.float32(0.99), zero_frames=0):
    """(out, block_max) of the reference's limiter on the whole stream `mix` ([frames] or [frames, channels]).
    zero_frames: that many frames of silence in front, cut from the result again -- what Limiter::skip amounts to;
    block_max then belongs to the stream with the silence in front."""
    x = np.asarray(mix, np.float32)
    if zero_frames:
        x = np.concatenate([np.zeros((zero_frames,) + x.shape[1:], np.float32), x])
    bm = block_maxima(x, block_size, ceiling)
    return ramp(x, 0, bm, block_size, 0, ceiling)[zero_frames:], bm


def _floor(n, ch, seed):
    return np.random.default_rng(seed).uniform(-FLOOR, FLOOR, (n, ch)).astype(np.float32)


def dynamics(ch, block_size, tail=777, seed=1):
    """Material D: 7 BS + tail frames.  Block maxima [0.99, 3, 1.5, 0.99, 0.99, 0.99, 0.995, 2.5]: a loud first sample of a block,
    a loud last sample of a block, blocks under the ceiling (block 4 and both its neighbours: its ramp is the identity (1, 0),
    the ramps of 3 and 5 are not), a block just over the ceiling, and the stream's last sample in a partial block"""
    BS = block_size
    assert tail >= 1
    x = _floor(7 * BS + tail, ch, seed)
    x[BS, 0] = 3.0
    x[3 * BS - 1, ch - 1] = -1.5
    x[6 * BS + BS // 2, 0] = 0.995
    x[-1, ch - 1] = -2.5
    return x


def ladder(n_blocks=17, ch=2, block_size=44100, tail=300, seed=2):
    """Material L: n_blocks BS + tail frames; on both sides of every boundary k = 1 .. n_blocks a peak, +-(1.20 + 0.02 j) for
    j = 2 k at sample k BS - 1 and j = 2 k + 1 at sample k BS, the sign alternating with j and the channel too: the last channel
    before the boundary, channel 0 behind it -- the two VALUES next to the boundary in the interleaved stream, for the kernels that
    count values and not frames.  The peaks rise strictly, so a boundary sample counted in the neighbouring block -- in either
    direction -- changes a block maximum by 0.02"""
    BS = block_size
    assert tail >= 1
    x = _floor(n_blocks * BS + tail, ch, seed)
    for k in range(1, n_blocks + 1):
        for j, s in ((2 * k, k * BS - 1), (2 * k + 1, k * BS)):
            x[s, 0 if j % 2 else ch - 1] = (1.20 + 0.02 * j) * (-1) ** j
    return x


def peak_at_end(n, ch, seed=3):
    """n frames of the floor with -2.5 on the very last sample: the stream's maximum in a last block of any length down to one sample"""
    x = _floor(n, ch, seed)
    x[-1, ch - 1] = -2.5
    return x


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
