#!/usr/bin/env python3
"""`get` of N stereo clips of 30 s that are resident as SIGNED 16-BIT PCM, as a decoder hands them out.

  gpu_get_batch_s16.py [out.json] [n_max] [--counts 64,1024]

Two ways to the same pattern lists, each a host clock around calls that end in a synchronise, both warmed up first, REPEATS repeats with
the two alternating inside each repeat, reported as median (min - max):

  a   what a caller did before: one awm_pcm_decode_d per clip into float buffers of its own (allocated once, outside the clock), then
      awm_get_watermark_batch_rates_d (or its keys form) on those
  b   awm_get_watermark_batch_rates_s16_d (or its keys form) on the 16-bit clips

for the first 64 and for all n_max (default 1024) clips of four sets: all at 48 kHz or the six rates mixed (drawn with a fixed seed), every
clip marked with the default key or with a key of its own (then decoded with that key per clip).

Memory, per way: the caller's buffers that hold the clips (16-bit; for a also the float copies) and what the context allocates for the
call after awm_ctx_trim (the sum of its grow-only buffers' requests, awm_debug_alloc_bytes; a buffer that grows twice counts twice), with
awm_debug_lane_pcm_bytes -- the float copies b keeps of clips -- beside it.  Also: a and b compared clip by clip (they must be equal) and
the payloads found."""
import ctypes as C
import json
import os
import statistics
import sys
import time

RATES = (44100, 48000, 32000, 96000, 22050, 88200)
SECONDS = 30
REPEATS = 5
SEED = 20240611
PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def main(path, n_max, counts):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import numpy as np
    import torch
    import audiowmark_amd as awm
    lib = awm.lib
    lib.awm_debug_alloc_bytes.restype = C.c_ulonglong
    ctx = awm.Context(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    keys = [awm.test_key(1 + i) for i in range(n_max)]
    mixed = [RATES[k] for k in np.random.default_rng(SEED).integers(0, len(RATES), n_max)]
    out = {"device": torch.cuda.get_device_name(0), "n_max": n_max, "seconds": SECONDS, "channels": 2, "repeats": REPEATS, "seed": SEED, "sets": {}}

    for set_name, rates, keyed in (("48k", [48000] * n_max, False), ("48k_keys", [48000] * n_max, True),
                                   ("mixed", mixed, False), ("mixed_keys", mixed, True)):
        clips16 = []
        for i, r in enumerate(rates):
            x = (torch.rand((SECONDS * r, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
            w = ctx.add_watermark(keys[i] if keyed else None, PAY1 if i % 2 else PAY2, x, sample_rate=r)
            clips16.append(ctx.pcm_encode(w.view(-1), 16, 0, False, True).view(torch.int16).view(w.shape))
        del x, w
        ctx.synchronize()
        floats = [torch.empty(c.shape, dtype=torch.float32, device="cuda") for c in clips16]      # a's copies: the caller's, allocated once
        torch.cuda.empty_cache()
        for n in counts:
            c16, fl, rs, ks = clips16[:n], floats[:n], rates[:n], keys[:n]
            results = {}

            def leg_a():
                for c, f in zip(c16, fl):
                    ctx.pcm_decode(c.view(-1).view(torch.uint8), 16, out=f.view(-1))
                results["a"] = ctx.get_watermark_batch_keys(ks, fl, sample_rate=rs) if keyed else ctx.get_watermark_batch(None, fl, sample_rate=rs)

            def leg_b():
                results["b"] = ctx.get_watermark_batch_keys_s16(ks, c16, sample_rate=rs) if keyed else ctx.get_watermark_batch_s16(None, c16, sample_rate=rs)

            legs = (("a", leg_a), ("b", leg_b))
            times = {"a": [], "b": []}
            for rep in range(-1, REPEATS):                      # -1: the warm-up of both
                for name, fn in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep >= 0:
                        times[name].append((time.perf_counter() - t0) * 1e3)
            memory = {}
            for name, fn in legs:                               # what the context allocates for one call, from nothing
                ctx.synchronize()
                assert lib.awm_ctx_trim(ctx._h) == 0
                before = lib.awm_debug_alloc_bytes()
                fn()
                ctx.synchronize()
                clip_bytes = sum(c.numel() * 2 for c in c16) + (sum(f.numel() * 4 for f in fl) if name == "a" else 0)
                memory[name] = {"caller_clip_bytes": clip_bytes, "context_bytes": int(lib.awm_debug_alloc_bytes() - before),
                                "lane_float_copies_bytes": int(lib.awm_debug_lane_pcm_bytes(ctx._h))}
                memory[name]["total_bytes"] = memory[name]["caller_clip_bytes"] + memory[name]["context_bytes"]
            want = [PAY1 if i % 2 else PAY2 for i in range(n)]
            entry = {"legs": {k: summary(v) for k, v in times.items()}, "memory": memory, "equal": results["a"] == results["b"],
                     "payloads_found": {k: sum(any(p["bits"] == pay for p in r) for r, pay in zip(results[k], want)) for k in results}}
            a, b = entry["legs"]["a"], entry["legs"]["b"]
            entry["b_minus_a_median_ms"] = b["median_ms"] - a["median_ms"]
            entry["a_spread_ms"] = a["max_ms"] - a["min_ms"]
            out["sets"].setdefault(set_name, {})[str(n)] = entry
            print("%-10s n=%-5d a %9.3f ms (%.3f - %.3f)   b %9.3f ms (%.3f - %.3f)   equal %s   found %s" %
                  (set_name, n, a["median_ms"], a["min_ms"], a["max_ms"], b["median_ms"], b["min_ms"], b["max_ms"], entry["equal"],
                   entry["payloads_found"]), flush=True)
            print("           memory a: clips %.3f GB + context %.3f GB   b: clips %.3f GB + context %.3f GB (float copies of clips: %d bytes)" %
                  (memory["a"]["caller_clip_bytes"] / 1e9, memory["a"]["context_bytes"] / 1e9, memory["b"]["caller_clip_bytes"] / 1e9,
                   memory["b"]["context_bytes"] / 1e9, memory["b"]["lane_float_copies_bytes"]), flush=True)
            with open(path, "w") as fh:                         # (after every entry: a run that is cut short leaves what it measured)
                json.dump(out, fh, indent=1)
                fh.write("\n")
        del clips16, floats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] in ("-h", "--help"):
        sys.exit(__doc__)
    counts = None
    if "--counts" in args:
        k = args.index("--counts")
        counts = [int(v) for v in args[k + 1].split(",")]
        del args[k:k + 2]
    n_max = int(args[1]) if len(args) > 1 else 1024
    path = args[0] if args else "get_batch_s16.json"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    main(path, n_max, counts or sorted({min(64, n_max), n_max}))
