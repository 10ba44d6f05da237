#!/usr/bin/env python3
"""A batch of stream segments at 48 kHz (awm_add_watermark_segments_rate_d) against what a caller had before it and against the 44.1 kHz path.

  gpu_add_segments_rate.py [timing.json]
      256 and 1024 stereo 48 kHz segments of 6 s + 2 x 3072 samples (slices of one resident buffer of uniform noise x 0.98: every limiter
      block ramps), a distinct payload each:
        window        one Context.add_watermark_segments (..., sample_rate=48000), zero_frames on multiples of 1024 around 600 s
        window_z0     the same batch at zero_frames = 0 for every segment
        window_far    the same batch one period of the pipeline (2 605 056 000 samples) + 600 s into the stream
        loop_z3072    per segment: "3072 zeros, then the segment" written to a scratch stream, awm_add_watermark_d at 48 kHz over it, the
                      segment's part copied out -- the only device-pointer route before this entry point, at an offset that flatters it
        loop_600s     the same at zero_frames = 600 s, for 16 segments only (what a server would actually pay per request)
        floor         awm_add_watermark_segments_d at 44.1 kHz: the same number of segments and samples, a distinct payload each
        subscribers   the new call for n subscribers of 16 distinct segments (segments that agree share one down-resampled slice)
      Host clock around calls that end in awm_ctx_synchronize.  Per repeat the legs run one after the other (interleaved), warm-up then
      timed steps; a leg's figure per repeat is the median of its steps, the table has the median and min - max of the repeats' figures.
      The window outputs at zero_frames = 3072 are compared with the loop's bit for bit.  After the timing, one profiled call of `window`
      gives the time per stage (the context's awm_prof_* scopes).
        hour_window / hour_whole   one 60 min stream that continues 100 samples in: the window form of one segment (K10w over a single
                      slice) against the whole-stream add of "100 zeros, then the stream" (the 147/160 phase kernels); outputs compared"""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RATE = 48000
SEG = 6 * RATE + 2 * 3072
COUNTS = [256, 1024]
PERIOD = 2605056000
Z600 = 600 * RATE // 1024 * 1024


def payloads(n):
    return ["%032x" % (0x0123456789abcdef0011223344556677 ^ (i * 0x9e3779b97f4a7c15f39cc0605cedc835 % (1 << 128))) for i in range(n)]


def timed(fn, steps):
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def leg_stats(per_repeat):
    return {"median_ms": statistics.median(per_repeat), "min_ms": min(per_repeat), "max_ms": max(per_repeat), "per_repeat_ms": per_repeat}


def main(path, counts=COUNTS, repeats=3):
    import torch
    import audiowmark_amd as awm
    from audiowmark_amd.binding import _hip_memcpy_dtod
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    ctx = awm.Context(0)
    n_max = max(counts)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    pool = ((torch.rand((n_max * SEG, 2), generator=g, device="cuda") * 2 - 1) * 0.98).contiguous()
    out_pool = torch.empty_like(pool)
    loop_pool = torch.empty_like(pool)
    # scratch of the loop legs, one stream per offset: the zeros in front are written once and stay zeros
    stream_in = {z: torch.zeros((z + SEG, 2), device="cuda") for z in (3072, 600 * RATE)}
    stream_out = {z: torch.empty_like(v) for z, v in stream_in.items()}
    result = {"segment_frames": SEG, "sample_rate": RATE, "channels": 2, "repeats": repeats, "device": torch.cuda.get_device_name(0), "rows": {}}
    for n in counts:
        pays = payloads(n)
        segs = [pool[i * SEG:(i + 1) * SEG] for i in range(n)]
        outs = [out_pool[i * SEG:(i + 1) * SEG] for i in range(n)]
        loop_outs = [loop_pool[i * SEG:(i + 1) * SEG] for i in range(n)]
        spread = [(i * 37 % 4000) * 1024 for i in range(n)]
        zfs = [Z600 + s for s in spread]
        zfs_far = [PERIOD + z for z in zfs]
        esz = 8

        def window(offsets=zfs):
            ctx.add_watermark_segments(None, pays, segs, offsets, outs, sample_rate=RATE)
            ctx.synchronize()

        def loop(z, count):
            for i in range(count):
                _hip_memcpy_dtod(ctx, stream_in[z].data_ptr() + z * esz, segs[i].data_ptr(), SEG * esz)
                ctx.add_watermark(None, pays[i], stream_in[z], stream_out[z], sample_rate=RATE)
                _hip_memcpy_dtod(ctx, loop_outs[i].data_ptr(), stream_out[z].data_ptr() + z * esz, SEG * esz)
            ctx.synchronize()

        def floor():
            ctx.add_watermark_segments(None, pays, segs, spread, outs)
            ctx.synchronize()

        def subscribers():
            ctx.add_watermark_segments(None, pays, [segs[i % 16] for i in range(n)], [zfs[i % 16] for i in range(n)], outs, sample_rate=RATE)
            ctx.synchronize()

        legs = [("window", window, 2, 5), ("window_z0", lambda: window([0] * n), 2, 5), ("window_far", lambda: window(zfs_far), 2, 5),
                ("loop_z3072", lambda: loop(3072, n), 1, 2), ("loop_600s", lambda: loop(600 * RATE, 16), 1, 2), ("floor", floor, 2, 5),
                ("subscribers", subscribers, 2, 5)]
        figures = {name: [] for name, _, _, _ in legs}
        fused_in_use = None
        for r in range(repeats):
            for name, fn, warmup, steps in legs:
                timed(fn, warmup)
                figures[name].append(statistics.median(timed(fn, steps)))
                if name == "window":
                    fused_in_use = awm.add_segments_fused_in_use()
        # the outputs: window == loop at zero_frames 3072
        window([3072] * n)
        loop(3072, n)
        equal = all(torch.equal(a, b) for a, b in zip(outs, loop_outs))
        # time per stage of one `window` call
        lib.awm_prof_enable(ctx._h, 1)
        lib.awm_prof_reset(ctx._h)
        window()
        stages = {}
        for i in range(lib.awm_prof_count()):
            ms, launches = C.c_double(), C.c_long()
            lib.awm_prof_read(ctx._h, i, C.byref(ms), C.byref(launches), None)
            if launches.value:
                stages[lib.awm_prof_name(i).decode()] = {"ms": ms.value, "launches": launches.value}
        lib.awm_prof_enable(ctx._h, 0)
        row = {name: leg_stats(v) for name, v in figures.items()}
        row.update(fused_in_use=fused_in_use, outputs_equal_z3072=equal, stages=stages,
                   loop_z3072_over_window=row["loop_z3072"]["median_ms"] / row["window"]["median_ms"],
                   loop_600s_per_segment_over_window_per_segment=(row["loop_600s"]["median_ms"] / 16) / (row["window"]["median_ms"] / n),
                   window_over_floor=row["window"]["median_ms"] / row["floor"]["median_ms"],
                   window_ms_per_segment=row["window"]["median_ms"] / n)
        result["rows"][str(n)] = row
        for name, _, _, _ in legs:
            s = row[name]
            print("n=%4d  %-12s %10.3f ms (%.3f - %.3f)" % (n, name, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
        print("n=%4d  loop_z3072 / window x%.2f  window / floor x%.2f  fused in use %s  equal %s" % (
              n, row["loop_z3072_over_window"], row["window_over_floor"], fused_in_use, equal), flush=True)
        print("n=%4d  stages of one window call: %s" % (n, ", ".join("%s %.3f ms / %d" % (k, v["ms"], v["launches"]) for k, v in stages.items())), flush=True)
        with open(path, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    # one long stream that continues 100 samples in (what the file level does with zero_frames at another rate): the window form of ONE
    # segment -- K10w over a single slice -- against the whole-stream add of "100 zeros, then the stream" (K10's 147/160 phase kernels)
    del pool, out_pool, loop_pool
    hour = 3600 * RATE
    g.manual_seed(8)
    s = torch.zeros((100 + hour, 2), device="cuda")
    s[100:] = (torch.rand((hour, 2), generator=g, device="cuda") * 2 - 1) * 0.98
    x, w_whole, w_window = s[100:], torch.empty_like(s), torch.empty((hour, 2), device="cuda")
    pay = payloads(1)[0]

    def hour_window():
        ctx.add_watermark_segments(None, [pay], [x], [100], [w_window], sample_rate=RATE)
        ctx.synchronize()

    def hour_whole():
        ctx.add_watermark(None, pay, s, w_whole, sample_rate=RATE)
        ctx.synchronize()

    figures = {"hour_window": [], "hour_whole": []}
    for r in range(repeats):
        for name, fn in (("hour_window", hour_window), ("hour_whole", hour_whole)):
            timed(fn, 2)
            figures[name].append(statistics.median(timed(fn, 5)))
    result["hour"] = {name: leg_stats(v) for name, v in figures.items()}
    result["hour"]["outputs_equal"] = bool(torch.equal(w_window, w_whole[100:]))
    for name, v in figures.items():
        st = result["hour"][name]
        print("60 min   %-12s %10.3f ms (%.3f - %.3f)" % (name, st["median_ms"], st["min_ms"], st["max_ms"]), flush=True)
    print("60 min   outputs equal %s" % result["hour"]["outputs_equal"], flush=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("-h", "--help"):
        sys.exit(__doc__)
    main(sys.argv[1] if len(sys.argv) > 1 else "timing.json")
