#!/usr/bin/env python3
"""`get` of ONE long stereo stream that is resident as SIGNED 16-BIT PCM, as a decoder or a WAV file hands it out.

  gpu_get_stream_s16.py [out.json] [--minutes 60,480]

Two ways to the same pattern list, each a host clock around calls that end in a synchronise, both warmed up first, REPEATS repeats with
the two alternating inside each repeat, reported as median (min - max):

  a   what a caller did before: awm_pcm_decode_d of the stream into a float buffer of its own (allocated once, outside the clock), then
      awm_get_watermark_d on that
  b   awm_get_watermark_s16_d on the 16-bit stream

for 60 min and 8 h of marked noise (the 8 h stream is the 60 min stream eight times over).

Memory, per way: the caller's buffers that hold the stream (16-bit; for a also the float copy), what the context allocates for the call
after awm_ctx_trim (the sum of its grow-only buffers' requests, awm_debug_alloc_bytes), and awm_debug_lane_pcm_bytes -- float copies of
PCM on the lanes, which b must not make.  Also: a and b compared (they must be equal) and how often the payload was found."""
import ctypes as C
import json
import os
import statistics
import sys
import time

REPEATS = 5
BASE_MINUTES = 60
PAYLOAD = "0123456789abcdef0011223344556677"


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def main(path, minutes):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch
    import audiowmark_amd as awm
    lib = awm.lib
    lib.awm_debug_alloc_bytes.restype = C.c_ulonglong
    ctx = awm.Context(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    x = (torch.rand((BASE_MINUTES * 60 * 44100, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
    w = ctx.add_watermark(None, PAYLOAD, x)
    base16 = ctx.pcm_encode(w.view(-1), 16, 0, False, True).view(torch.int16).view(w.shape)
    del x, w
    ctx.synchronize()
    torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "channels": 2, "repeats": REPEATS, "streams": {}}
    for m in minutes:
        reps, rest = divmod(m, BASE_MINUTES)
        parts = [base16] * reps + ([base16[: rest * 60 * 44100]] if rest else [])
        s16 = torch.cat(parts).contiguous() if len(parts) > 1 else parts[0]
        f32 = torch.empty(s16.shape, dtype=torch.float32, device="cuda")          # a's copy: the caller's, allocated once
        results = {}

        def leg_a():
            ctx.pcm_decode(s16.view(-1).view(torch.uint8), 16, out=f32.view(-1))
            results["a"] = ctx.get_watermark(None, f32)

        def leg_b():
            results["b"] = ctx.get_watermark_s16(None, s16)

        legs = (("a", leg_a), ("b", leg_b))
        times = {"a": [], "b": []}
        for rep in range(-1, REPEATS):                          # -1: the warm-up of both
            for name, fn in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep >= 0:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        memory = {}
        for name, fn in legs:                                   # what the context allocates for one call, from nothing
            ctx.synchronize()
            assert lib.awm_ctx_trim(ctx._h) == 0
            before = lib.awm_debug_alloc_bytes()
            fn()
            ctx.synchronize()
            held = s16.numel() * 2 + (f32.numel() * 4 if name == "a" else 0)
            memory[name] = {"caller_stream_bytes": held, "context_bytes": int(lib.awm_debug_alloc_bytes() - before),
                            "lane_float_copies_bytes": int(lib.awm_debug_lane_pcm_bytes(ctx._h))}
            memory[name]["total_bytes"] = memory[name]["caller_stream_bytes"] + memory[name]["context_bytes"]
        entry = {"frames": int(s16.shape[0]), "legs": {k: summary(v) for k, v in times.items()}, "memory": memory,
                 "equal": results["a"] == results["b"], "patterns": len(results["b"]),
                 "payload_found": {k: sum(p["bits"] == PAYLOAD for p in results[k]) for k in results}}
        a, b = entry["legs"]["a"], entry["legs"]["b"]
        entry["b_minus_a_median_ms"] = b["median_ms"] - a["median_ms"]
        entry["a_spread_ms"] = a["max_ms"] - a["min_ms"]
        entry["bar_met"] = entry["b_minus_a_median_ms"] <= entry["a_spread_ms"]
        out["streams"]["%d_min" % m] = entry
        print("%4d min   a %9.3f ms (%.3f - %.3f)   b %9.3f ms (%.3f - %.3f)   equal %s   payload found %s   bar met %s" %
              (m, a["median_ms"], a["min_ms"], a["max_ms"], b["median_ms"], b["min_ms"], b["max_ms"], entry["equal"], entry["payload_found"],
               entry["bar_met"]), flush=True)
        print("           memory a: stream %.3f GB + context %.3f GB   b: stream %.3f GB + context %.3f GB (float copies on the lanes: %d bytes)" %
              (memory["a"]["caller_stream_bytes"] / 1e9, memory["a"]["context_bytes"] / 1e9, memory["b"]["caller_stream_bytes"] / 1e9,
               memory["b"]["context_bytes"] / 1e9, memory["b"]["lane_float_copies_bytes"]), flush=True)
        with open(path, "w") as fh:                             # (after every entry: a run that is cut short leaves what it measured)
            json.dump(out, fh, indent=1)
            fh.write("\n")
        del s16, f32, parts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] in ("-h", "--help"):
        sys.exit(__doc__)
    minutes = [60, 480]
    if "--minutes" in args:
        k = args.index("--minutes")
        minutes = [int(v) for v in args[k + 1].split(",")]
        del args[k:k + 2]
    path = args[0] if args else "get_stream_s16.json"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    main(path, minutes)
