"""The file level and the command line on the tile stream at 48 kHz (add_stream_watermark -> add_tiles -> awm_add_stream_create_rate_at,
DESIGN.md section 9.5): the bytes written are those of awm_add_watermark_d on the whole stream, encoded with pcm_encode; the device memory
of a call does not depend on the length of the file; a pipe of unknown length is written like the file; --snr keeps the whole-stream path
and its figure."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AWM = os.path.join(ROOT, "audiowmark_amd", "audiowmark")
PAY = "0123456789abcdef0011223344556677"
R48 = 48000


def wav_header(n_bytes, rate=R48, channels=2, bits=16):
    return b"RIFF" + struct.pack("<I", 36 + n_bytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * channels * bits // 8,
                                                                                   channels * bits // 8, bits) + b"data" + struct.pack("<I", n_bytes)


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
    g.cache = {}

    def material(seconds):
        """(s16 bytes, the samples a reader decodes from them, the whole-stream add of those) of `seconds` of noise x 0.9 at 48 kHz stereo"""
        if seconds not in g.cache:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(40 + seconds)
            n = seconds * R48 + 77
            x = ((torch.rand((n, 2), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1) * 0.9).contiguous()
            pcm = ctx.pcm_encode(x.reshape(-1), 16, 0, False, True)
            x_file = ctx.pcm_decode(pcm, 16, 0, False).reshape(n, 2)
            whole = ctx.add_watermark(None, PAY, x_file, sample_rate=R48)
            ctx.synchronize()
            g.cache[seconds] = (pcm.cpu().numpy().tobytes(), x_file, whole)
        return g.cache[seconds]
    g.material = material
    yield g
    g.cache.clear()
    ctx.close()


def file_add(gpu, src, dst, raw=None):
    """add_watermark_file on a context of its own -> device bytes the call allocated"""
    awm = gpu.awm
    ctx = awm.Context(0)
    try:
        ctx.synchronize()
        before = awm.lib.awm_debug_alloc_bytes()
        ctx.add_watermark_file(None, PAY, src, dst, raw, raw)
        return awm.lib.awm_debug_alloc_bytes() - before
    finally:
        ctx.close()


def test_wav_files_of_100_s_and_300_s(gpu, tmp_path):
    allocated = {}
    for seconds in (100, 300):
        pcm, _, whole = gpu.material(seconds)
        src, dst = tmp_path / f"in{seconds}.wav", tmp_path / f"out{seconds}.wav"
        src.write_bytes(wav_header(len(pcm)) + pcm)
        allocated[seconds] = file_add(gpu, src, dst)
        # (a named WAV file: samples are clipped at 32 bit and the top 16 bits kept, tests/test_gpu_streaming.py)
        want = gpu.ctx.pcm_encode(whole.reshape(-1), 16, 0, False, False).cpu().numpy().tobytes()
        out = dst.read_bytes()
        assert out[:44] == wav_header(len(pcm)) and out[44:] == want, seconds
    print("device bytes allocated by the call: 100 s: %d, 300 s: %d" % (allocated[100], allocated[300]))
    # bounded memory: three times the stream, the same bytes (whole in HBM, the 300 s call needs 200 s x 48000 x 8 bytes x 4 buffers more)
    assert allocated[300] == allocated[100]


def test_a_raw_pipe_of_unknown_length_through_the_command_line(gpu, tmp_path):
    pcm, _, whole = gpu.material(100)
    rf = gpu.awm.binding.RawFormat(2, R48, 16, 0, 0)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(pcm)
    file_add(gpu, src, dst, rf)
    want = gpu.ctx.pcm_encode(whole.reshape(-1), 16, 0, False, True).cpu().numpy().tobytes()      # (the raw writer's 16 bit rule)
    assert dst.read_bytes() == want
    r = subprocess.run([AWM, "add", "--input-format", "raw", "--raw-rate", "48000", "--output-format", "raw", "-", "-", PAY], input=pcm,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == dst.read_bytes()


def test_snr_keeps_the_whole_stream_path_and_its_figure(gpu, tmp_path):
    pcm, x_file, whole = gpu.material(100)
    src, dst = tmp_path / "in.wav", tmp_path / "out.wav"
    src.write_bytes(wav_header(len(pcm)) + pcm)
    r = subprocess.run([AWM, "add", "--snr", str(src), str(dst), PAY], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in (r.stderr + b"\n" + r.stdout).decode(errors="replace").splitlines() if l.startswith("SNR:")]
    assert len(lines) == 1, lines
    gpu.ctx.snr_begin()
    gpu.ctx.add_watermark(None, PAY, x_file, sample_rate=R48)
    figure = gpu.ctx.snr_end()
    assert abs(float(lines[0].split()[1]) - figure) < 1e-5, (lines, figure)       # (printed with six decimals; sums of doubles in any order)
    want = gpu.ctx.pcm_encode(whole.reshape(-1), 16, 0, False, False).cpu().numpy().tobytes()
    assert dst.read_bytes()[44:] == want
