#!/usr/bin/env python3
"""A request queue at six sample rates: one mixed call (awm_add_watermark_segments_rates_d) against the queue sorted by
rate and one one-rate call per rate.

  gpu_add_segments_rates.py [timing.json] [sorted]
      256 and 1024 stereo requests of 6 s + 2 x 3072 samples at their own rate (slices of resident buffers of uniform noise x 0.98: every
      limiter block ramps), zero_frames on multiples of 1024 around ten minutes in, a distinct payload each, the six rates 48 / 32 / 96 /
      22.05 / 88.2 / 44.1 kHz in equal shares, shuffled (seeded):
        mixed         one Context.add_watermark_segments (..., sample_rate=[a rate per request])
        sorted        the requests grouped by rate (the grouping itself is not timed), one add_watermark_segments per rate: the only
                      route before the mixed call, through code that the mixed call does not change
        mixed_keys / sorted_keys      the same with 16 keys (add_watermark_segments_keys)
        mixed_s16 / sorted_s16        the same from and to 16-bit PCM (add_watermark_segments_s16)
      `sorted` as the second argument runs the sorted legs alone (they exist on a tree without the mixed call).
      Host clock around calls that end in awm_ctx_synchronize.  Per repeat the legs run one after the other, warm-up then timed steps; a
      leg's figure per repeat is the median of its steps, the table has the median and min - max of the three repeats' figures.  The
      outputs of each pair of legs are compared bit for bit.  After the timing: the time until the mixed call and the six one-rate calls
      RETURN (the host's share; the synchronise behind them is not timed), and one profiled call of `mixed` and of `sorted` for the time
      per stage (the context's awm_prof_* scopes)."""
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RATES = [48000, 32000, 96000, 22050, 88200, 44100]
COUNTS = [256, 1024]


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


def main(path, sorted_only=False, counts=COUNTS, repeats=3):
    import torch
    import audiowmark_amd as awm
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    ctx = awm.Context(0)
    n_max = max(counts)
    rates_all = [RATES[i % 6] for i in range(n_max)]
    random.Random(7).shuffle(rates_all)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    seg_len = {r: 6 * r + 2 * 3072 for r in RATES}
    total = sum(seg_len[r] for r in rates_all)
    pool = ((torch.rand((total, 2), generator=g, device="cuda") * 2 - 1) * 0.98).contiguous()
    pool16 = torch.round(pool * 32767).to(torch.int16).contiguous()
    out_a, out_b = torch.empty_like(pool), torch.empty_like(pool)
    out16_a, out16_b = torch.empty_like(pool16), torch.empty_like(pool16)
    starts = [0]
    for r in rates_all:
        starts.append(starts[-1] + seg_len[r])               # (every slice begins on the 16-byte grid: the lengths are even)
    key16 = [awm.test_key(100 + k) for k in range(16)]
    result = {"rates": RATES, "channels": 2, "repeats": repeats, "device": torch.cuda.get_device_name(0), "sorted_only": sorted_only, "rows": {}}

    def stages_of(fn):
        lib.awm_prof_enable(ctx._h, 1)
        lib.awm_prof_reset(ctx._h)
        fn()
        stages = {}
        for i in range(lib.awm_prof_count()):
            ms, launches = C.c_double(), C.c_long()
            lib.awm_prof_read(ctx._h, i, C.byref(ms), C.byref(launches), None)
            if launches.value:
                stages[lib.awm_prof_name(i).decode()] = {"ms": ms.value, "launches": launches.value}
        lib.awm_prof_enable(ctx._h, 0)
        return stages

    for n in counts:
        rates = rates_all[:n]
        pays = payloads(n)
        keys = [key16[i % 16] for i in range(n)]
        cut = lambda t: [t[starts[i]:starts[i + 1]] for i in range(n)]
        segs, segs16 = cut(pool), cut(pool16)
        outs_a, outs_b, outs16_a, outs16_b = cut(out_a), cut(out_b), cut(out16_a), cut(out16_b)
        zfs = [600 * rates[i] // 1024 * 1024 + (i * 37 % 4000) * 1024 for i in range(n)]
        by_rate = {r: [i for i in range(n) if rates[i] == r] for r in RATES}
        pick = lambda v, idx: [v[i] for i in idx]
        groups = {r: dict(pays=pick(pays, idx), keys=pick(keys, idx), zfs=pick(zfs, idx), segs=pick(segs, idx), segs16=pick(segs16, idx),
                          outs=pick(outs_b, idx), outs16=pick(outs16_b, idx)) for r, idx in by_rate.items()}

        def mixed():
            ctx.add_watermark_segments(None, pays, segs, zfs, outs_a, sample_rate=rates)
            ctx.synchronize()

        def mixed_keys():
            ctx.add_watermark_segments_keys(keys, pays, segs, zfs, outs_a, sample_rate=rates)
            ctx.synchronize()

        def mixed_s16():
            ctx.add_watermark_segments_s16(None, pays, segs16, zfs, outs16_a, sample_rate=rates)
            ctx.synchronize()

        def by_rate_calls():
            for r, q in groups.items():
                ctx.add_watermark_segments(None, q["pays"], q["segs"], q["zfs"], q["outs"], sample_rate=r)
            ctx.synchronize()

        def by_rate_keys():
            for r, q in groups.items():
                ctx.add_watermark_segments_keys(q["keys"], q["pays"], q["segs"], q["zfs"], q["outs"], sample_rate=r)
            ctx.synchronize()

        def by_rate_s16():
            for r, q in groups.items():
                ctx.add_watermark_segments_s16(None, q["pays"], q["segs16"], q["zfs"], q["outs16"], sample_rate=r)
            ctx.synchronize()

        pairs = [("", mixed, by_rate_calls, outs_a, outs_b), ("_keys", mixed_keys, by_rate_keys, outs_a, outs_b),
                 ("_s16", mixed_s16, by_rate_s16, outs16_a, outs16_b)]
        legs = []
        for tag, m, s, _, _ in pairs:
            if not sorted_only:
                legs.append(("mixed" + tag, m))
            legs.append(("sorted" + tag, s))
        figures = {name: [] for name, _ in legs}
        for r in range(repeats):
            for name, fn in legs:
                timed(fn, 2)
                figures[name].append(statistics.median(timed(fn, 5)))
        row = {name: leg_stats(v) for name, v in figures.items()}
        # the host's share: the time until the call (the six calls) returned, the synchronise behind it not timed -- the one-rate calls
        # prepare the next rate while the device works on the previous one, the mixed call prepares everything before its first launch
        def enqueue_ms(call):
            out = []
            for _ in range(7):
                t0 = time.perf_counter()
                call()
                out.append((time.perf_counter() - t0) * 1e3)
                ctx.synchronize()
            return statistics.median(out[2:])
        if not sorted_only:
            row["mixed_enqueue_ms"] = enqueue_ms(lambda: ctx.add_watermark_segments(None, pays, segs, zfs, outs_a, sample_rate=rates))
        row["sorted_enqueue_ms"] = enqueue_ms(lambda: [ctx.add_watermark_segments(None, q["pays"], q["segs"], q["zfs"], q["outs"], sample_rate=r)
                                                       for r, q in groups.items()])
        print("n=%4d  enqueue alone: mixed %s ms, sorted %.3f ms" % (n, "%.3f" % row["mixed_enqueue_ms"] if not sorted_only else "-",
                                                                    row["sorted_enqueue_ms"]), flush=True)
        if not sorted_only:
            for tag, m, s, a, b in pairs:
                m()
                fused = awm.add_segments_fused_in_use()
                s()
                row["outputs_equal" + tag] = all(torch.equal(x, y) for x, y in zip(a, b))
                row["fused_in_use" + tag] = fused
                row["sorted_over_mixed" + tag] = row["sorted" + tag]["median_ms"] / row["mixed" + tag]["median_ms"]
            row["stages_mixed"] = stages_of(mixed)
        row["stages_sorted"] = stages_of(by_rate_calls)
        result["rows"][str(n)] = row
        for name, _ in legs:
            s = row[name]
            print("n=%4d  %-12s %10.3f ms (%.3f - %.3f)" % (n, name, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
        if not sorted_only:
            print("n=%4d  sorted / mixed x%.3f  keys x%.3f  s16 x%.3f  fused in use %s %s %s  equal %s %s %s" % (
                  n, row["sorted_over_mixed"], row["sorted_over_mixed_keys"], row["sorted_over_mixed_s16"], row["fused_in_use"],
                  row["fused_in_use_keys"], row["fused_in_use_s16"], row["outputs_equal"], row["outputs_equal_keys"], row["outputs_equal_s16"]),
                  flush=True)
        for which in ("stages_mixed", "stages_sorted"):
            if which in row:
                print("n=%4d  %s: %s" % (n, which, ", ".join("%s %.3f ms / %d" % (k, v["ms"], v["launches"]) for k, v in row[which].items())),
                      flush=True)
        with open(path, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("-h", "--help"):
        sys.exit(__doc__)
    main(sys.argv[1] if len(sys.argv) > 1 else "timing.json", sorted_only=len(sys.argv) > 2 and sys.argv[2] == "sorted")
