#!/usr/bin/env python3
"""One input at 48 kHz, many payloads: awm_add_watermark_payloads_d with the shared down-resample against a loop of
awm_add_watermark_d.  The script uses nothing but what the tree before this path had as well unless it is asked to, so that the baseline
can be a build of that tree: run `loop` there and `call` here, on the same box, one after the other.

  gpu_add_payloads_rate.py loop [out.json]
      60 min stereo at 48 kHz resident in HBM (uniform noise at +-1: every limiter block ramps); P in 2, 4, 8: P single-payload calls
      into P buffers.  One warm-up, then 7 timed runs, each bracketed by events on the stream; the figure is their median.  With the
      per-id breakdown of awm_prof_read from one further run.
  gpu_add_payloads_rate.py call [out.json] [mode ...]
      the same for ONE awm_add_watermark_payloads_d call in the modes given (default: 2 1), awm_debug_set_add_payloads_rate_fused;
      the outputs of the modes are compared with a loop's (torch.equal).
  gpu_add_payloads_rate.py files DIR [out.json]
      a 16 bit stereo WAV of the hour at 48 kHz to 4 files through awm_add_watermark_payloads_file: wall time of 3 calls."""
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RATE = 48000
N = 60 * 60 * RATE
PS = [2, 4, 8]
RUNS = 7


def payloads(n):
    return ["%032x" % (0x0123456789abcdef0011223344556677 ^ (i * 0x9e3779b97f4a7c15f39cc0605cedc835 % (1 << 128))) for i in range(n)]


def material(torch, n=N):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    return (torch.rand((n, 2), generator=g, device="cuda") * 2 - 1).contiguous()


def timed(torch, fn, ctx):
    """one warm-up, then RUNS runs between two events each -> (median, min, max, all) in ms"""
    fn()
    ctx.synchronize()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ctx.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def breakdown(awm, ctx, fn):
    """per profiling id of one run: launches, ms and algorithmic bytes (awm_prof_read)"""
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    ctx.synchronize()
    lib.awm_prof_enable(ctx._h, 1)
    try:
        lib.awm_prof_reset(ctx._h)
        fn()
        ctx.synchronize()
        out = {}
        for i in range(lib.awm_prof_count()):
            ms, launches, nbytes = C.c_double(), C.c_long(), C.c_double()
            lib.awm_prof_read(ctx._h, i, C.byref(ms), C.byref(launches), C.byref(nbytes))
            if launches.value:
                out[lib.awm_prof_name(i).decode()] = {"launches": launches.value, "ms": ms.value, "algorithmic_bytes": nbytes.value}
    finally:
        lib.awm_prof_enable(ctx._h, 0)
    return out


def run(kind, path, modes):
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    x = material(torch)
    bufs = [torch.empty_like(x) for _ in range(max(PS))]
    result = {"kind": kind, "rate": RATE, "n_frames": N, "channels": 2, "runs": RUNS, "device": torch.cuda.get_device_name(0), "rows": {}}
    for P in PS:
        pays = payloads(P)

        def loop():
            for p in range(P):
                ctx.add_watermark(None, pays[p], x, out=bufs[p], sample_rate=RATE)
        if kind == "loop":
            row = timed(torch, loop, ctx)
            row["prof"] = breakdown(awm, ctx, loop)
            result["rows"]["P%d" % P] = row
            print("loop    P=%d  %8.3f ms (%.3f - %.3f)" % (P, row["median_ms"], row["min_ms"], row["max_ms"]), flush=True)
            continue
        loop()
        ctx.synchronize()
        want = [b.clone() for b in bufs[:P]]
        for mode in modes:
            awm.set_add_payloads_rate_fused(mode)

            def call():
                ctx.add_watermark_payloads(None, pays, x, bufs[:P], sample_rate=RATE)
            row = timed(torch, call, ctx)
            row["path_in_use"] = awm.add_payloads_rate_fused_in_use()
            row["outputs_equal_loop"] = all(torch.equal(bufs[p], want[p]) for p in range(P))
            row["prof"] = breakdown(awm, ctx, call)
            result["rows"]["P%d_mode%d" % (P, mode)] = row
            print("mode %d  P=%d  %8.3f ms (%.3f - %.3f)  path %d  equal %s" % (mode, P, row["median_ms"], row["min_ms"], row["max_ms"],
                                                                                 row["path_in_use"], row["outputs_equal_loop"]), flush=True)
        awm.set_add_payloads_rate_fused(2)
        del want
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


def run_files(root, path):
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    os.makedirs(root, exist_ok=True)
    src = os.path.join(root, "hour48.wav")
    x = material(torch)
    pcm = ctx.pcm_encode(x.reshape(-1), 16, 0, False, True).cpu().numpy()
    del x
    with open(src, "wb") as fh:
        n_bytes = pcm.nbytes
        fh.write(b"RIFF" + struct.pack("<I", 36 + n_bytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, RATE, RATE * 4, 4, 16)
                 + b"data" + struct.pack("<I", n_bytes))
        fh.write(pcm.tobytes())
    del pcm
    pays = payloads(4)
    dsts = [os.path.join(root, "out%d.wav" % p) for p in range(4)]
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.add_watermark_payloads_file(None, pays, src, dsts)
        wall.append(time.perf_counter() - t0)
        print("files  P=4  %.3f s" % wall[-1], flush=True)
    result = {"kind": "files", "rate": RATE, "n_frames": N, "payloads": 4, "wall_s": wall, "median_s": statistics.median(wall)}
    for p in [src] + dsts:
        os.remove(p)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode in ("loop", "call"):
        run(mode, sys.argv[2] if len(sys.argv) > 2 else mode + ".json", [int(m) for m in sys.argv[3:]] or [2, 1])
    elif mode == "files" and len(sys.argv) > 2:
        run_files(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "files.json")
    else:
        sys.exit(__doc__)
