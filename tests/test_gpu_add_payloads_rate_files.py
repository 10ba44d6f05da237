"""One input FILE, many payloads at a sample rate other than 44.1 kHz (awm_add_watermark_payloads_file / awm_add_stream_watermark_payloads_file):
the input goes to HBM once, the outputs are produced there in passes of at most four -- awm_add_watermark_payloads_d for a stream that starts
at sample 0, awm_add_watermark_segments_rate_d with aliased inputs for one that continues zero_frames samples in -- and written one after
the other.  Every file is byte for byte what add_watermark_file writes for that payload (filecmp): there is no tolerance."""
import filecmp
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SECONDS = 8
FORMATS = {"wav_s16_stereo": (2, 16, 0, False, True), "raw_s24be_mono": (1, 24, 0, True, False)}

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def payloads(n, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = rng.integers(0, 256, 16, dtype=np.uint8).tobytes().hex()
        if p not in out:
            out.append(p)
    return out


def wav_header(n_bytes, channels, rate, bits):
    return b"RIFF" + struct.pack("<I", 36 + n_bytes) + b"WAVEfmt " \
        + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits) + b"data" + struct.pack("<I", n_bytes)


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
    yield g
    _CACHE.clear()
    awm.set_add_payloads_rate_fused(2)
    awm.set_params()
    ctx.close()


@pytest.fixture(scope="module")
def files(gpu, tmp_path_factory):
    """the input file of a format and rate (written once) and the file add_watermark_file writes for a payload (once per payload and zero_frames)"""
    root = tmp_path_factory.mktemp("payload_rate_files")
    torch = gpu.torch

    class F:
        pass
    f = F()

    def source(fmt, rate):
        ch, bits, enc, big, wav = FORMATS[fmt]

        def make():
            gen = torch.Generator(device="cuda")
            gen.manual_seed(90 + ch)
            n = SECONDS * rate + 123
            x = (torch.rand((n, ch) if ch > 1 else (n,), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).contiguous()
            pcm = gpu.ctx.pcm_encode(x.reshape(-1), bits, enc, big, True).cpu().numpy().tobytes()
            path = root / ("in_%s_%d.%s" % (fmt, rate, "wav" if wav else "raw"))
            with open(path, "wb") as out:
                out.write((wav_header(len(pcm), ch, rate, bits) if wav else b"") + pcm)
            return path, (None if wav else gpu.awm.binding.RawFormat(ch, rate, bits, enc, int(big)))
        return cached(("source", fmt, rate), make)
    f.source = source

    def single(fmt, rate, pay, zero_frames):
        def make():
            src, rf = source(fmt, rate)
            dst = root / ("single_%s_%d_%s_%s" % (fmt, rate, pay, zero_frames))
            gpu.ctx.add_watermark_file(None, pay, src, dst, rf, rf, zero_frames=zero_frames)
            return dst
        return cached(("single file", fmt, rate, pay, zero_frames), make)
    f.single = single
    return f


def check_files(gpu, files, tmp_path, fmt, rate, n_pay, zero_frames):
    pays = payloads(n_pay)
    src, rf = files.source(fmt, rate)
    dsts = [tmp_path / ("out%d" % p) for p in range(n_pay)]
    gpu.ctx.add_watermark_payloads_file(None, pays, src, dsts, rf, rf, zero_frames=zero_frames)
    path = gpu.awm.add_payloads_rate_fused_in_use()
    for p, pay in enumerate(pays):
        assert os.path.getsize(dsts[p]) == os.path.getsize(src)
        assert filecmp.cmp(dsts[p], files.single(fmt, rate, pay, zero_frames), shallow=False), f"file {p} of {n_pay} differs from add_watermark_file's"
    assert not filecmp.cmp(dsts[0], dsts[1], shallow=False)
    return path


@pytest.mark.parametrize("zero_frames", [None, 1115])
def test_wav_s16_stereo_48_khz(gpu, files, tmp_path, zero_frames):
    """five payloads: passes of 3 + 2 over output buffers that are reused"""
    path = check_files(gpu, files, tmp_path, "wav_s16_stereo", 48000, 5, zero_frames)
    if zero_frames is None:
        assert path == 2


def test_raw_s24be_mono_32_khz(gpu, files, tmp_path):
    assert check_files(gpu, files, tmp_path, "raw_s24be_mono", 32000, 3, None) == 1


def test_the_switch_off_gives_the_same_files(gpu, files, tmp_path):
    gpu.awm.set_add_payloads_rate_fused(0)
    try:
        assert check_files(gpu, files, tmp_path, "wav_s16_stereo", 48000, 2, None) == 0
    finally:
        gpu.awm.set_add_payloads_rate_fused(2)
