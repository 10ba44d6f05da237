#!/usr/bin/env python3
"""One input, many payloads: the fused call (awm_add_watermark_payloads_d, kernel K2m) against a loop of awm_add_watermark_d.

  gpu_add_payloads.py time [timing.json]
      60 min stereo at 44.1 kHz resident in HBM, uniform noise at +-1 (every limiter block ramps) and at +-0.25 (the limiter's apply
      pass skips everything); P in 1, 2, 4, 8, 16.  fused = one call into P buffers, loop = P single-payload calls into P other
      buffers, both ending in awm_ctx_synchronize.  Per repeat: 3 warm-up + 20 timed steps of the one leg, then of the other; five
      repeats, the legs trading their buffers from repeat to repeat.  A leg's figure per repeat is the median of its 20 steps; the
      table has the median and min - max of the five figures.  The outputs of the last steps are compared with torch.equal.
  gpu_add_payloads.py prof [P]
      a few steps of the fused call with P (default 8) payloads and of the single call, for `rocprofv3 --kernel-trace --stats` and for
      the `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes (counters in runs of their own)
  gpu_add_payloads.py summary timing.json kernel_stats.csv fetch_counter_collection.csv write_counter_collection.csv
      adds the kernels' own durations and their HBM traffic over the algorithmic bytes to timing.json"""
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N = 60 * 60 * 44100
STREAM_BYTES = N * 2 * 4
PS = [1, 2, 4, 8, 16]
WARMUP, STEPS, REPEATS = 3, 20, 5
HBM_PEAK = 8e12


def payloads(n):
    return ["%032x" % (0x0123456789abcdef0011223344556677 ^ (i * 0x9e3779b97f4a7c15f39cc0605cedc835 % (1 << 128))) for i in range(n)]


def material(torch, amp):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    return ((torch.rand((N, 2), generator=g, device="cuda") * 2 - 1) * amp).contiguous()


def timed(fn, ctx, steps):
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def leg_stats(per_repeat):
    return {"median_ms": statistics.median(per_repeat), "min_ms": min(per_repeat), "max_ms": max(per_repeat), "per_repeat_ms": per_repeat}


def run_time(path):
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    result = {"n_frames": N, "channels": 2, "stream_bytes": STREAM_BYTES, "warmup": WARMUP, "steps": STEPS, "repeats": REPEATS,
              "tile": awm.ADD_PAYLOADS_TILE, "device": torch.cuda.get_device_name(0), "materials": {}}
    fused_bufs = [torch.empty((N, 2), dtype=torch.float32, device="cuda") for _ in range(max(PS))]
    loop_bufs = [torch.empty((N, 2), dtype=torch.float32, device="cuda") for _ in range(max(PS))]
    for name, amp in (("noise_1.0", 1.0), ("noise_0.25", 0.25)):
        x = material(torch, amp)
        rows = {}
        for P in PS:
            pays = payloads(P)

            def fused():
                ctx.add_watermark_payloads(None, pays, x, fused_bufs[:P])

            def loop():
                for p in range(P):
                    ctx.add_watermark(None, pays[p], x, out=loop_bufs[p])
            fused_med, loop_med = [], []
            for r in range(REPEATS):
                if r:
                    fused_bufs, loop_bufs = loop_bufs, fused_bufs          # the legs trade buffers: where a buffer lies in HBM is in both legs' spread
                timed(fused, ctx, WARMUP)
                fused_med.append(statistics.median(timed(fused, ctx, STEPS)))
                in_use = awm.add_payloads_fused_in_use()
                timed(loop, ctx, WARMUP)
                loop_med.append(statistics.median(timed(loop, ctx, STEPS)))
            equal = all(torch.equal(fused_bufs[p], loop_bufs[p]) for p in range(P))
            f, l = leg_stats(fused_med), leg_stats(loop_med)
            rows[str(P)] = {"fused": f, "loop": l, "fused_in_use": in_use, "outputs_equal": equal,
                            "fused_ms_per_output": f["median_ms"] / P, "loop_ms_per_output": l["median_ms"] / P,
                            "loop_over_fused": l["median_ms"] / f["median_ms"],
                            "fused_median_below_loop_min": f["median_ms"] < l["min_ms"],
                            "fused_median_within_loop_range": l["min_ms"] <= f["median_ms"] <= l["max_ms"]}
            print("%-10s P=%2d  fused %8.3f ms (%.3f - %.3f)  loop %8.3f ms (%.3f - %.3f)  per output %.3f / %.3f ms  x%.2f  equal %s" % (
                  name, P, f["median_ms"], f["min_ms"], f["max_ms"], l["median_ms"], l["min_ms"], l["max_ms"], f["median_ms"] / P, l["median_ms"] / P,
                  l["median_ms"] / f["median_ms"], equal), flush=True)
        result["materials"][name] = rows
        del x
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


def run_prof(P):
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    x = material(torch, 1.0)
    pays = payloads(P)
    outs = [torch.empty_like(x) for _ in range(P)]
    for _ in range(3):
        ctx.add_watermark_payloads(None, pays, x, outs)
        ctx.add_watermark(None, pays[0], x, out=outs[0])
    ctx.synchronize()
    print("prof: P = %d, fused in use %d" % (P, awm.add_payloads_fused_in_use()))


def short_name(name):
    name = name.replace("(anonymous namespace)::", "")
    return name.split("awmk::")[1].split("(")[0] if "awmk::" in name else None


def run_summary(timing, stats_csv, fetch_csv, write_csv):
    with open(timing) as fh:
        result = json.load(fh)
    kernels = {}
    with open(stats_csv, newline="") as fh:
        for row in csv.DictReader(fh):
            k = short_name(row["Name"])
            if k:
                kernels.setdefault(k, {})["calls"] = int(row["Calls"])
                kernels[k]["average_ms"] = float(row["AverageNs"]) / 1e6
                kernels[k]["min_ms"] = float(row["MinNs"]) / 1e6
                kernels[k]["max_ms"] = float(row["MaxNs"]) / 1e6
    # FETCH_SIZE / WRITE_SIZE in KiB; a coalesced 16 B / lane stream shows half its bytes in FETCH_SIZE on gfx950 (tools/pmc_traffic.py)
    for path, counter, scale, key in ((fetch_csv, "FETCH_SIZE", 2 * 1024, "fetch_bytes"), (write_csv, "WRITE_SIZE", 1024, "write_bytes")):
        acc = {}
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                k = short_name(row["Kernel_Name"])
                if k and row["Counter_Name"] == counter:
                    acc.setdefault(k, []).append(float(row["Counter_Value"]))
        for k, v in acc.items():
            kernels.setdefault(k, {})[key] = scale * sum(v) / len(v)
    stream = result["stream_bytes"]
    algorithmic = {"add_mix_multi_pair_kernel": (1 + result["tile"]) * stream, "add_mix_pair_kernel": 2 * stream}      # P = 8: two passes of a full tile
    for k, alg in algorithmic.items():
        e = kernels.get(k)
        if e and "fetch_bytes" in e and "write_bytes" in e:
            e["algorithmic_bytes"] = alg
            e["traffic_over_algorithmic"] = (e["fetch_bytes"] + e["write_bytes"]) / alg
            if "average_ms" in e:
                e["fraction_of_8TBps"] = alg / (e["average_ms"] * 1e-3) / HBM_PEAK
    result["kernels_P8"] = {k: v for k, v in sorted(kernels.items()) if k.startswith(("add_mix", "limiter", "fill"))}
    with open(timing, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["kernels_P8"], indent=1))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode == "time":
        run_time(sys.argv[2] if len(sys.argv) > 2 else "timing.json")
    elif mode == "prof":
        run_prof(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
    elif mode == "summary":
        run_summary(*sys.argv[2:6])
    else:
        sys.exit(__doc__)
