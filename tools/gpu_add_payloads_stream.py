#!/usr/bin/env python3
"""One input, many payloads with bounded memory: the tile stream with P payloads and the file level call against loops of their
single-payload forms (awm_add_stream_create_payloads_at / awm_add_watermark_payloads_file; kernel: K2m's span form).

  gpu_add_payloads_stream.py tiles [timing.json]
      60 min stereo at 44.1 kHz resident in HBM, tile 4096 frames, uniform noise at +-1 (every limiter block ramps) and at +-0.25;
      P in 2, 4, 8.  fused = one Context.add_watermark_payloads_tiles, loop = P Context.add_watermark_tiles, both ending in
      awm_ctx_synchronize (both include the object's creation and the copies of the tiles in and out, as a caller of the tile stream
      pays them).  Per repeat: warm-up + timed steps of the one leg, then of the other; a leg's figure per repeat is the median of its
      steps, the table has the median and min - max of the repeats' figures.  The outputs of the last steps are compared.
  gpu_add_payloads_stream.py files [timing.json] [directory]
      a 60 min 16 bit stereo WAV in `directory` (default: /dev/shm, a tmpfs); fused = one awm_add_watermark_payloads_file, loop = P
      awm_add_watermark_file into the same P paths; P in 2, 4, 8.  Host clock around the calls (they return when the files are closed).
      The files of the last steps are compared by their SHA-1.
  gpu_add_payloads_stream.py prof [P]
      a few fused tile streams with P (default 4) payloads and single ones, for `rocprofv3 --kernel-trace --stats`
  gpu_add_payloads_stream.py summary timing.json kernel_stats.csv
      adds the kernels' own durations to timing.json
Both timing modes merge their section into timing.json if it exists."""
import csv
import hashlib
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N = 60 * 60 * 44100
TILE = 4096
PS = [2, 4, 8]


def payloads(n):
    return ["%032x" % (0x0123456789abcdef0011223344556677 ^ (i * 0x9e3779b97f4a7c15f39cc0605cedc835 % (1 << 128))) for i in range(n)]


def material(torch, amp, n=N):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    return ((torch.rand((n, 2), generator=g, device="cuda") * 2 - 1) * amp).contiguous()


def timed(fn, steps):
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def leg_stats(per_repeat):
    return {"median_ms": statistics.median(per_repeat), "min_ms": min(per_repeat), "max_ms": max(per_repeat), "per_repeat_ms": per_repeat}


def row_of(f, l, P, **more):
    row = {"fused": f, "loop": l, "fused_ms_per_output": f["median_ms"] / P, "loop_ms_per_output": l["median_ms"] / P,
           "loop_over_fused": l["median_ms"] / f["median_ms"], "fused_median_below_loop_min": f["median_ms"] < l["min_ms"],
           "fused_median_within_loop_range": l["min_ms"] <= f["median_ms"] <= l["max_ms"]}
    row.update(more)
    return row


def show(name, P, row):
    f, l = row["fused"], row["loop"]
    print("%-10s P=%2d  fused %9.3f ms (%.3f - %.3f)  loop %9.3f ms (%.3f - %.3f)  per output %.3f / %.3f ms  x%.2f  equal %s" % (
          name, P, f["median_ms"], f["min_ms"], f["max_ms"], l["median_ms"], l["min_ms"], l["max_ms"], row["fused_ms_per_output"],
          row["loop_ms_per_output"], row["loop_over_fused"], row["outputs_equal"]), flush=True)


def merge(path, section, value):
    result = {}
    if os.path.exists(path):
        with open(path) as fh:
            result = json.load(fh)
    result[section] = value
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


def run_tiles(path, n=N, warmup=2, steps=8, repeats=3):
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    result = {"n_frames": n, "channels": 2, "tile_frames1024": TILE, "warmup": warmup, "steps": steps, "repeats": repeats,
              "outputs_per_pass": awm.ADD_PAYLOADS_TILE, "device": torch.cuda.get_device_name(0), "materials": {}}
    for name, amp in (("noise_1.0", 1.0), ("noise_0.25", 0.25)):
        x = material(torch, amp, n)
        rows = {}
        for P in PS:
            pays = payloads(P)
            keep = {}

            def fused():
                keep["fused"] = ctx.add_watermark_payloads_tiles(None, pays, x, TILE)

            def loop():
                keep["loop"] = [ctx.add_watermark_tiles(None, p, x, TILE) for p in pays]
            fused_med, loop_med = [], []
            for r in range(repeats):
                timed(fused, warmup)
                fused_med.append(statistics.median(timed(fused, steps)))
                in_use = awm.add_payloads_fused_in_use()
                timed(loop, warmup)
                loop_med.append(statistics.median(timed(loop, steps)))
            equal = all(torch.equal(a, b) for a, b in zip(keep["fused"], keep["loop"]))
            rows[str(P)] = row_of(leg_stats(fused_med), leg_stats(loop_med), P, fused_in_use=in_use, outputs_equal=equal)
            show(name, P, rows[str(P)])
            keep.clear()
        result["materials"][name] = rows
        del x
    merge(path, "tile_stream", result)


def wav_header(n_bytes, channels=2, rate=44100, bits=16):
    return b"RIFF" + struct.pack("<I", 36 + n_bytes) + b"WAVEfmt " \
        + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits) + b"data" + struct.pack("<I", n_bytes)


def sha1(path):
    h = hashlib.sha1()
    with open(path, "rb") as fh:
        for block in iter(lambda: fh.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def run_files(path, directory, n=N, warmup=1, steps=3, repeats=3):
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    awm.lib.awm_set_quiet(1)
    work = tempfile.mkdtemp(prefix="awm_payloads_", dir=directory)
    try:
        src = os.path.join(work, "in.wav")
        pcm = ctx.pcm_encode(material(torch, 1.0, n).reshape(-1), 16, 0, False, True).cpu().numpy()
        with open(src, "wb") as fh:
            fh.write(wav_header(pcm.nbytes))
            pcm.tofile(fh)
        del pcm
        torch.cuda.empty_cache()
        result = {"n_frames": n, "channels": 2, "format": "WAV, 16 bit", "input_bytes": os.path.getsize(src), "directory": directory,
                  "warmup": warmup, "steps": steps, "repeats": repeats, "device": torch.cuda.get_device_name(0), "rows": {}}
        for P in PS:
            pays = payloads(P)
            dsts = [os.path.join(work, "out%d.wav" % p) for p in range(P)]

            def fused():
                ctx.add_watermark_payloads_file(None, pays, src, dsts)

            def loop():
                for p in range(P):
                    ctx.add_watermark_file(None, pays[p], src, dsts[p])
            fused_med, loop_med = [], []
            for r in range(repeats):
                timed(fused, warmup)
                fused_med.append(statistics.median(timed(fused, steps)))
                in_use = awm.add_payloads_fused_in_use()
                if r == repeats - 1:
                    fused_sums = [sha1(d) for d in dsts]
                timed(loop, warmup)
                loop_med.append(statistics.median(timed(loop, steps)))
            equal = fused_sums == [sha1(d) for d in dsts] and len(set(fused_sums)) == P
            result["rows"][str(P)] = row_of(leg_stats(fused_med), leg_stats(loop_med), P, fused_in_use=in_use, outputs_equal=equal)
            show("wav 16 bit", P, result["rows"][str(P)])
            for d in dsts:
                os.remove(d)
        merge(path, "file_level", result)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def run_prof(P):
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    x = material(torch, 1.0)
    pays = payloads(P)
    for _ in range(3):
        ctx.add_watermark_payloads_tiles(None, pays, x, TILE)
        ctx.add_watermark_tiles(None, pays[0], x, TILE)
    ctx.synchronize()
    print("prof: P = %d, fused in use %d" % (P, awm.add_payloads_fused_in_use()))


def short_name(name):
    name = name.replace("(anonymous namespace)::", "")
    return name.split("awmk::")[1].split("(")[0] if "awmk::" in name else None


def run_summary(timing, stats_csv):
    kernels = {}
    with open(stats_csv, newline="") as fh:
        for row in csv.DictReader(fh):
            k = short_name(row["Name"])
            if k and k.startswith(("add_mix", "limiter", "fill")):
                kernels[k] = {"calls": int(row["Calls"]), "average_ms": float(row["AverageNs"]) / 1e6, "min_ms": float(row["MinNs"]) / 1e6,
                              "max_ms": float(row["MaxNs"]) / 1e6}
    merge(timing, "kernels_per_tile_4096", dict(sorted(kernels.items())))
    print(json.dumps(kernels, indent=1))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "tiles"
    out = sys.argv[2] if len(sys.argv) > 2 else "timing.json"
    if mode == "tiles":
        run_tiles(out)
    elif mode == "files":
        run_files(out, sys.argv[3] if len(sys.argv) > 3 else "/dev/shm")
    elif mode == "prof":
        run_prof(int(sys.argv[2]) if len(sys.argv) > 2 else 4)
    elif mode == "summary":
        run_summary(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
