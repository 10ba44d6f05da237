#!/usr/bin/env python3
"""The tile stream at 48 kHz (awm_add_stream_create_rate_at) against the whole-stream add.  Host clock around calls
that end in a synchronise; three repeats, the legs alternating within a repeat; the figure is the median (min - max).

  gpu_add_stream_rate.py resident [out.json]
      60 min stereo at 48 kHz resident in HBM (uniform noise at +-1: every limiter block ramps), outputs into resident buffers:
        whole     awm_add_watermark_d
        tiles     the object, tile 4096 frames, the span phase kernels (K10s)
        tiles_w   the same with awm_debug_set_resample_phase (0): K10w
      and for 4 payloads: four one-payload objects one after the other against one four-payload object.
  gpu_add_stream_rate.py file DIR AUDIOWMARK [AUDIOWMARK ...] [out.json]
      the hour as a 16 bit stereo WAV at 48 kHz through `AUDIOWMARK add` of every binary given (first this build, then a build of the
      tree before this path): wall time of the process, three alternating runs each; the outputs of the binaries are compared byte for byte.
  gpu_add_stream_rate.py bytes DIR [out.json]
      device bytes one awm_add_watermark_file call of that WAV asks for (awm_debug_alloc_bytes), on a fresh context."""
import json
import os
import statistics
import struct
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RATE = 48000
N = 60 * 60 * RATE
TILE_FRAMES = 4096
REPEATS = 3
PAY = "0123456789abcdef0011223344556677"


def payloads(n):
    return ["%032x" % (0x0123456789abcdef0011223344556677 ^ (i * 0x9e3779b97f4a7c15f39cc0605cedc835 % (1 << 128))) for i in range(n)]


def material(torch, n=N):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    return (torch.rand((n, 2), generator=g, device="cuda") * 2 - 1).contiguous()


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def alternate(legs, ctx):
    """legs: {name: fn}; one warm-up of each, then REPEATS rounds over all of them -> {name: summary in ms}"""
    for fn in legs.values():
        fn()
    ctx.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(REPEATS):
        for name, fn in legs.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: summary(v) for name, v in ms.items()}


def run_resident(path):
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    x = material(torch)
    pays = payloads(4)
    result = {"kind": "resident", "rate": RATE, "n_frames": N, "tile_frames1024": TILE_FRAMES, "repeats": REPEATS,
              "device": torch.cuda.get_device_name(0)}
    out = torch.empty_like(x)
    ctx.add_watermark(None, PAY, x, out=out, sample_rate=RATE)
    ctx.synchronize()
    want = out.clone()
    kept = {}

    def tiles(phase):
        def fn():
            awm.lib.awm_debug_set_resample_phase(phase)
            try:
                kept[phase] = ctx.add_watermark_tiles(None, PAY, x, TILE_FRAMES, sample_rate=RATE)
            finally:
                awm.lib.awm_debug_set_resample_phase(1)
        return fn
    one = alternate({"whole": lambda: ctx.add_watermark(None, PAY, x, out=out, sample_rate=RATE), "tiles": tiles(1), "tiles_w": tiles(0)}, ctx)
    one["equal"] = bool(torch.equal(kept[1], want) and torch.equal(kept[0], want))
    result["one_payload"] = one
    for name in ("whole", "tiles", "tiles_w"):
        print("%-8s %9.3f ms (%.3f - %.3f)" % (name, one[name]["median"], one[name]["min"], one[name]["max"]), flush=True)
    kept.clear()
    del want

    def four_objects():
        for p in pays:
            kept["last"] = ctx.add_watermark_tiles(None, p, x, TILE_FRAMES, sample_rate=RATE)

    def one_object():
        kept["outs"] = ctx.add_watermark_payloads_tiles(None, pays, x, TILE_FRAMES, sample_rate=RATE)
    four = alternate({"four_objects": four_objects, "one_object": one_object}, ctx)
    four["equal"] = bool(torch.equal(kept["outs"][-1], kept["last"]))
    result["four_payloads"] = four
    for name in ("four_objects", "one_object"):
        print("%-12s %9.3f ms (%.3f - %.3f)" % (name, four[name]["median"], four[name]["min"], four[name]["max"]), flush=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


def write_hour(root):
    import torch
    import audiowmark_amd as awm
    os.makedirs(root, exist_ok=True)
    src = os.path.join(root, "hour48.wav")
    ctx = awm.Context(0)
    pcm = ctx.pcm_encode(material(torch).reshape(-1), 16, 0, False, True).cpu().numpy()
    with open(src, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 36 + pcm.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, RATE, RATE * 4, 4, 16)
                 + b"data" + struct.pack("<I", pcm.nbytes))
        fh.write(pcm.tobytes())
    ctx.close()
    return src


def run_file(root, binaries, path):
    src = write_hour(root)
    wall = {b: [] for b in binaries}
    digests = {}
    for r in range(REPEATS + 1):                             # (round 0 warms the page cache and the binaries)
        for i, b in enumerate(binaries):
            dst = os.path.join(root, "out%d.wav" % i)
            t0 = time.perf_counter()
            subprocess.run([b, "add", "-q", src, dst, PAY], check=True, stdout=subprocess.DEVNULL)
            dt = time.perf_counter() - t0
            if r:
                wall[b].append(dt)
            print("%s  %.3f s%s" % (b, dt, "" if r else "  (warm-up)"), flush=True)
            with open(dst, "rb") as fh:
                import hashlib
                digests[b] = hashlib.sha1(fh.read()).hexdigest()
            os.remove(dst)
    os.remove(src)
    labels = {b: "this_build" if i == 0 else "parent_build" if i == 1 else "build%d" % i for i, b in enumerate(binaries)}
    result = {"kind": "file", "rate": RATE, "n_frames": N, "repeats": REPEATS, "wall_s": {labels[b]: summary(v) for b, v in wall.items()},
              "outputs_equal": len(set(digests.values())) == 1}
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


def run_bytes(root, path):
    import audiowmark_amd as awm
    src = write_hour(root)
    dst = os.path.join(root, "out.wav")
    ctx = awm.Context(0)
    ctx.synchronize()
    before = awm.lib.awm_debug_alloc_bytes()
    ctx.add_watermark_file(None, PAY, src, dst)
    asked = awm.lib.awm_debug_alloc_bytes() - before
    ctx.close()
    os.remove(src)
    os.remove(dst)
    print("device bytes asked for by the call: %d" % asked, flush=True)
    with open(path, "w") as fh:
        json.dump({"kind": "bytes", "rate": RATE, "n_frames": N, "device_bytes": asked}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    args = sys.argv[2:]
    out = args.pop() if args and args[-1].endswith(".json") else mode + ".json"
    if mode == "resident":
        run_resident(out)
    elif mode == "file" and len(args) >= 2:
        run_file(args[0], args[1:], out)
    elif mode == "bytes" and len(args) == 1:
        run_bytes(args[0], out)
    else:
        sys.exit(__doc__)
