#!/usr/bin/env python3
"""Segment batches from and to signed 16-bit PCM (awm_add_watermark_segments_rate_s16_d) against what a caller
with resident 16-bit segments had before it.

  gpu_add_segments_s16.py [timing.json] [n_segments]
      n (1024) stereo segments of 6 s + 2 x 3072 samples, slices of one resident int16 buffer (uniform noise x 0.98: every limiter block
      ramps), a distinct payload each, zero_frames on multiples of 1024 around 600 s; at 44.1 kHz and at 48 kHz:
        s16      one Context.add_watermark_segments_s16 on the int16 segments, into int16 outputs
        before   per segment awm_pcm_decode_d into a float buffer, one Context.add_watermark_segments on the float buffers, per segment
                 awm_pcm_encode_d (direct16) into the int16 outputs: the same work with the entry points there were
        float    the float call of `before` alone (the floor)
      Host clock around legs that end in awm_ctx_synchronize.  Per repeat the legs run one after the other (interleaved), warm-up then
      timed steps; a leg's figure per repeat is the median of its steps, the table has the median and min - max of the repeats' figures.
      The outputs of s16 and before are compared value for value.  After the timing, one profiled run of s16 and of before gives the time
      per stage (the context's awm_prof_* scopes), and the bytes that stay resident for the segments on either side are printed.
  gpu_add_segments_s16.py prof [n_segments]
      three runs of s16 and of before at both rates and nothing else: what a `rocprofv3 --kernel-trace --stats` run wraps"""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RATES = [44100, 48000]


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


class Side:
    """the buffers and the three legs at one rate"""

    def __init__(self, torch, ctx, rate, n):
        self.ctx, self.rate, self.n = ctx, rate, n
        self.seg = 6 * rate + 2 * 3072
        g = torch.Generator(device="cuda")
        g.manual_seed(7 + rate)
        x = (torch.rand((n * self.seg, 2), generator=g, device="cuda") * 2 - 1) * 0.98
        self.pool16 = torch.round(x * 32767).to(torch.int16).contiguous()
        del x
        self.out16 = torch.zeros_like(self.pool16)
        self.out16_before = torch.zeros_like(self.pool16)
        self.pool_f = torch.empty((n * self.seg, 2), device="cuda", dtype=torch.float32)
        self.out_f = torch.empty_like(self.pool_f)
        cut = lambda t: [t[i * self.seg:(i + 1) * self.seg] for i in range(n)]
        self.segs16, self.outs16, self.outs16_before = cut(self.pool16), cut(self.out16), cut(self.out16_before)
        self.segs_f, self.outs_f = cut(self.pool_f), cut(self.out_f)
        self.raw_in = [s.view(torch.uint8).reshape(-1) for s in self.segs16]
        self.raw_out = [s.view(torch.uint8).reshape(-1) for s in self.outs16_before]
        self.pays = payloads(n)
        z600 = 600 * rate // 1024 * 1024
        self.zfs = [z600 + (i * 37 % 4000) * 1024 for i in range(n)]

    def s16(self):
        self.ctx.add_watermark_segments_s16(None, self.pays, self.segs16, self.zfs, self.outs16, sample_rate=self.rate)
        self.ctx.synchronize()

    def floor(self):
        self.ctx.add_watermark_segments(None, self.pays, self.segs_f, self.zfs, self.outs_f, sample_rate=self.rate)
        self.ctx.synchronize()

    def before(self):
        ctx = self.ctx
        for i in range(self.n):
            ctx.pcm_decode(self.raw_in[i], 16, out=self.segs_f[i].reshape(-1))
        ctx.add_watermark_segments(None, self.pays, self.segs_f, self.zfs, self.outs_f, sample_rate=self.rate)
        for i in range(self.n):
            ctx.pcm_encode(self.outs_f[i].reshape(-1), 16, direct16=True, out=self.raw_out[i])
        ctx.synchronize()

    def resident_bytes(self):
        values = self.n * self.seg * 2
        return {"s16": values * (2 + 2), "before": values * (2 + 4 + 4 + 2)}


def stages(lib, ctx, fn):
    lib.awm_prof_enable(ctx._h, 1)
    lib.awm_prof_reset(ctx._h)
    fn()
    out = {}
    for i in range(lib.awm_prof_count()):
        ms, launches = C.c_double(), C.c_long()
        lib.awm_prof_read(ctx._h, i, C.byref(ms), C.byref(launches), None)
        if launches.value:
            out[lib.awm_prof_name(i).decode()] = {"ms": ms.value, "launches": launches.value}
    lib.awm_prof_enable(ctx._h, 0)
    return out


def main(path, n, repeats=3):
    import torch
    import audiowmark_amd as awm
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    ctx = awm.Context(0)
    result = {"segments": n, "channels": 2, "repeats": repeats, "device": torch.cuda.get_device_name(0), "rates": {}}
    for rate in RATES:
        side = Side(torch, ctx, rate, n)
        legs = [("s16", side.s16, 2, 5), ("before", side.before, 1, 3), ("float", side.floor, 2, 5)]
        figures = {name: [] for name, _, _, _ in legs}
        fused = None
        for r in range(repeats):
            for name, fn, warmup, steps in legs:
                timed(fn, warmup)
                figures[name].append(statistics.median(timed(fn, steps)))
                if name == "s16":
                    fused = awm.add_segments_fused_in_use()
        side.s16()
        side.before()
        equal = bool(torch.equal(side.out16, side.out16_before))
        row = {name: leg_stats(v) for name, v in figures.items()}
        row.update(segment_frames=side.seg, fused_in_use=fused, outputs_equal=equal, resident_bytes=side.resident_bytes(),
                   stages_s16=stages(lib, ctx, side.s16), stages_before=stages(lib, ctx, side.before),
                   before_over_s16=row["before"]["median_ms"] / row["s16"]["median_ms"],
                   s16_over_float=row["s16"]["median_ms"] / row["float"]["median_ms"])
        result["rates"][str(rate)] = row
        for name, _, _, _ in legs:
            s = row[name]
            print("%5d Hz n=%4d  %-7s %10.3f ms (%.3f - %.3f)" % (rate, n, name, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
        print("%5d Hz  before / s16 x%.2f  s16 / float x%.2f  fused in use %s  outputs equal %s  resident bytes %s" % (
              rate, row["before_over_s16"], row["s16_over_float"], fused, equal, row["resident_bytes"]), flush=True)
        for which in ("stages_s16", "stages_before"):
            print("%5d Hz  %s: %s" % (rate, which, ", ".join("%s %.3f ms / %d" % (k, v["ms"], v["launches"]) for k, v in row[which].items())), flush=True)
        with open(path, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        del side
        torch.cuda.empty_cache()


def prof(n):
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    for rate in RATES:
        side = Side(torch, ctx, rate, n)
        for _ in range(3):
            side.s16()
            side.before()
        del side
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("-h", "--help"):
        sys.exit(__doc__)
    if len(sys.argv) > 1 and sys.argv[1] == "prof":
        prof(int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else "timing.json", int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
