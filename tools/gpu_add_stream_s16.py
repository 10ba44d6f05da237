#!/usr/bin/env python3
"""`add` of ONE long stereo stream that is resident as SIGNED 16-BIT PCM and wanted back as 16-bit PCM.

  gpu_add_stream_s16.py [out.json] [--minutes 60,480] [--rates 44100,48000]

Three ways, each a host clock around calls that end in a synchronise, all warmed up first, REPEATS repeats with the legs alternating inside
each repeat, reported as median (min - max):

  a   what a caller did before: awm_pcm_decode_d into a float buffer of its own, awm_add_watermark_d into a second one, awm_pcm_encode_d
      into the 16-bit output (the float buffers allocated once, outside the clock)
  b   awm_add_watermark_s16_d from the 16-bit stream into the 16-bit output
  f   the float call alone, awm_add_watermark_d on a's decoded copy (what the two conversions of a cost beside it)

and for "watermark, then verify": ga = decode + awm_add_get_watermark_d + encode, gb = awm_add_get_watermark_s16_d.

Streams: 60 min and 8 h of noise at 44.1 kHz (the 8 h stream is the 60 min stream eight times over); at another rate the hour alone.
Memory, per way: the caller's buffers that hold the stream, and what the context allocates for the call after awm_ctx_trim (the sum of its
grow-only buffers' requests, awm_debug_alloc_bytes).  Also: a and b compared (they must be equal), and how often ga and gb find the
payload.  (ga_equals_gb is recorded but not expected to hold: ga's `get` reads the float stream BEFORE its quantisation to 16 bits, gb's
the 16-bit output, so qualities and errors differ in their last digits; what gb's list equals is awm_get_watermark_rate_s16_d on the
output, which the tests hold.)"""
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


def main(path, minutes, rates):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch
    import audiowmark_amd as awm
    lib = awm.lib
    lib.awm_debug_alloc_bytes.restype = C.c_ulonglong
    ctx = awm.Context(0)
    out = {"device": torch.cuda.get_device_name(0), "channels": 2, "repeats": REPEATS, "streams": {}}
    for rate in rates:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        x = (torch.rand((BASE_MINUTES * 60 * rate, 2), generator=gen, device="cuda") - 0.5).contiguous()
        base16 = ctx.pcm_encode(x.view(-1), 16, 0, False, True).view(torch.int16).view(x.shape)
        del x
        ctx.synchronize()
        torch.cuda.empty_cache()
        for m in (minutes if rate == 44100 else minutes[:1]):
            reps, rest = divmod(m, BASE_MINUTES)
            parts = [base16] * reps + ([base16[: rest * 60 * rate]] if rest else [])
            s16 = torch.cat(parts).contiguous() if len(parts) > 1 else parts[0]
            f_in = torch.empty(s16.shape, dtype=torch.float32, device="cuda")        # a's float buffers: the caller's, allocated once
            f_out = torch.empty(s16.shape, dtype=torch.float32, device="cuda")
            o16 = {k: torch.empty_like(s16) for k in ("a", "b")}
            results = {}

            def decode():
                ctx.pcm_decode(s16.view(-1).view(torch.uint8), 16, out=f_in.view(-1))

            def encode(dst):
                ctx.pcm_encode(f_out.view(-1), 16, 0, False, True, out=dst.view(-1).view(torch.uint8))

            def leg_a():
                decode()
                ctx.add_watermark(None, PAYLOAD, f_in, f_out, sample_rate=rate)
                encode(o16["a"])

            def leg_b():
                ctx.add_watermark_s16(None, PAYLOAD, s16, o16["b"], sample_rate=rate)
                results["fused"] = lib.awm_debug_add_s16_fused_in_use()

            def leg_f():
                ctx.add_watermark(None, PAYLOAD, f_in, f_out, sample_rate=rate)

            def leg_ga():
                decode()
                results["ga"] = ctx.add_get_watermark(None, PAYLOAD, f_in, f_out, sample_rate=rate)
                encode(o16["a"])

            def leg_gb():
                results["gb"] = ctx.add_get_watermark_s16(None, PAYLOAD, s16, o16["b"], sample_rate=rate)

            legs = (("a", leg_a), ("b", leg_b), ("f", leg_f), ("ga", leg_ga), ("gb", leg_gb))
            times = {name: [] for name, _ in legs}
            for rep in range(-1, REPEATS):                          # -1: the warm-up of all
                for name, fn in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep >= 0:
                        times[name].append((time.perf_counter() - t0) * 1e3)
            leg_a()
            leg_b()
            ctx.synchronize()
            equal = bool(torch.equal(o16["a"], o16["b"]))
            memory = {}
            held = {"a": s16.numel() * (2 + 4 + 4 + 2), "b": s16.numel() * (2 + 2), "f": s16.numel() * (4 + 4),
                    "ga": s16.numel() * (2 + 4 + 4 + 2), "gb": s16.numel() * (2 + 2)}
            for name, fn in legs:                                   # what the context allocates for one call, from nothing
                ctx.synchronize()
                assert lib.awm_ctx_trim(ctx._h) == 0
                before = lib.awm_debug_alloc_bytes()
                fn()
                ctx.synchronize()
                memory[name] = {"caller_stream_bytes": held[name], "context_bytes": int(lib.awm_debug_alloc_bytes() - before)}
                memory[name]["total_bytes"] = memory[name]["caller_stream_bytes"] + memory[name]["context_bytes"]
            entry = {"rate": rate, "frames": int(s16.shape[0]), "legs": {k: summary(v) for k, v in times.items()}, "memory": memory,
                     "a_equals_b": equal, "b_fused": int(results["fused"]), "ga_equals_gb": results["ga"] == results["gb"],
                     "payload_found": {k: sum(p["bits"] == PAYLOAD for p in results[k]) for k in ("ga", "gb")}}
            out["streams"]["%d_min_%d" % (m, rate)] = entry
            L = entry["legs"]
            print("%4d min %6d Hz  " % (m, rate) + "   ".join("%s %9.3f ms (%.3f - %.3f)" % (k, L[k]["median_ms"], L[k]["min_ms"], L[k]["max_ms"])
                                                              for k in ("a", "b", "f", "ga", "gb")), flush=True)
            print("           a == b %s   fused %d   ga == gb %s   payload found %s   memory (caller + context, GB): " %
                  (equal, entry["b_fused"], entry["ga_equals_gb"], entry["payload_found"]) +
                  "  ".join("%s %.2f + %.2f" % (k, memory[k]["caller_stream_bytes"] / 1e9, memory[k]["context_bytes"] / 1e9) for k in memory), flush=True)
            with open(path, "w") as fh:                             # (after every entry: a run that is cut short leaves what it measured)
                json.dump(out, fh, indent=1)
                fh.write("\n")
            del s16, f_in, f_out, o16, parts
            torch.cuda.empty_cache()
        del base16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] in ("-h", "--help"):
        sys.exit(__doc__)
    minutes, rates = [60, 480], [44100, 48000]
    if "--minutes" in args:
        k = args.index("--minutes")
        minutes = [int(v) for v in args[k + 1].split(",")]
        del args[k:k + 2]
    if "--rates" in args:
        k = args.index("--rates")
        rates = [int(v) for v in args[k + 1].split(",")]
        del args[k:k + 2]
    path = args[0] if args else "add_stream_s16.json"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    main(path, minutes, rates)
