#!/usr/bin/env python3
"""`get --detect-speed` of N stereo clips of 30 s through awm_get_watermark_batch_d / ..._rates_s16_d.

  gpu_get_batch_speed.py [out.json] [n_max] [--counts 64,1024] [--only a,b,c] [--sets f44_tenth,...]

Three ways to the same pattern lists, timed in one process with a host clock around calls that end in a synchronise, every shape
warmed up first, REPEATS repeats with the ways alternating inside each repeat, reported as median (min - max):

  a   one clip after the other on the context's lane with the one-clip search: what the batches did under a speed parameter before
      (awm_debug_set_speed_batch (2), kept for this tool)
  b   every clip over the work lanes in parallel, each with the one-clip search (awm_debug_set_speed_batch (0), the default)
  c   the clips in their groups, the speed search of a group as a batch on the slices of stage 0, sub-groups in lockstep
      (awm_debug_set_speed_batch (1)), at the byte budgets of BUDGETS_GB (awm_debug_set_speed_batch_bytes): legs c_4g, c_12g, c_32g

Sets: float at 44.1 kHz and 16-bit at 48 kHz; a tenth of the clips replayed at 0.9764 or 1.01 and the rest at speed 1, or every clip
off speed.  Every clip is marked; the results of a, b and c are compared list for list."""
import json
import os
import statistics
import sys
import time

SECONDS = 30
REPEATS = 5
BUDGETS_GB = (4, 12, 32)
SPEEDS = (0.9764, 1.01)
PAY = "0123456789abcdef0011223344556677"


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def main(path, n_max, counts, only, sets):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch
    import audiowmark_amd as awm
    ctx = awm.Context(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    out = {"device": torch.cuda.get_device_name(0), "n_max": n_max, "seconds": SECONDS, "channels": 2, "repeats": REPEATS,
           "default_budget_bytes": awm.speed_batch_bytes(), "budgets_gb": list(BUDGETS_GB), "sets": {}}
    for set_name in sets:
        fmt, variant = set_name.split("_")
        rate = 44100 if fmt == "f44" else 48000
        clips = []
        for i in range(n_max):
            x = (torch.rand((SECONDS * rate, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
            w = ctx.add_watermark(None, PAY, x, sample_rate=rate)
            off = variant == "all" or i % 10 == 0
            if off:
                w = ctx.resample_ratio(w, 1 / SPEEDS[(i // 10 if variant == "tenth" else i) % 2], rate=rate)
            if fmt == "s48":
                w = ctx.pcm_encode(w.view(-1), 16, 0, False, True).view(torch.int16).view(w.shape)
            clips.append(w)
        del x, w
        ctx.synchronize()
        torch.cuda.empty_cache()
        for n in counts:
            cs = clips[:n]
            results = {}

            def leg(name, mode, budget_gb):
                def fn():
                    awm.set_speed_batch(mode)
                    awm.set_speed_batch_bytes(int(budget_gb * (1 << 30)))
                    results[name] = ctx.get_watermark_batch_s16(None, cs, sample_rate=rate) if fmt == "s48" else ctx.get_watermark_batch(None, cs)
                return name, fn
            legs = [leg("a", 2, 0), leg("b", 0, 0)] + [leg("c_%dg" % g, 1, g) for g in BUDGETS_GB]
            legs = [l for l in legs if l[0][0] in only]
            times = {name: [] for name, _ in legs}
            launches = {}
            awm.set_speed_params(detect_speed=True)
            try:
                for rep in range(-1, REPEATS):                      # -1: the warm-up of every way
                    for name, fn in legs:
                        torch.cuda.synchronize()
                        before = awm.speed_batch_launches()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        if rep >= 0:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                        launches[name] = [a - b for a, b in zip(awm.speed_batch_launches(), before)]
            finally:
                awm.set_speed_params()
                awm.set_speed_batch(0)
                awm.set_speed_batch_bytes(0)
            first = results[legs[0][0]]
            stretched = sum(any(p["bits"] == PAY and p["speed"] != 1 for p in r) for r in first)
            entry = {"legs": {k: summary(v) for k, v in times.items()}, "batch_kernel_launches": launches,
                     "equal": all(results[k] == first for k in results), "payload_found": sum(any(p["bits"] == PAY for p in r) for r in first),
                     "payload_found_stretched": stretched}
            out["sets"].setdefault(set_name, {})[str(n)] = entry
            print("%-10s n=%-5d %s   equal %s   found %d (%d stretched)" %
                  (set_name, n, "   ".join("%s %.2f ms (%.2f - %.2f)" % (k, v["median_ms"], v["min_ms"], v["max_ms"]) for k, v in entry["legs"].items()),
                   entry["equal"], entry["payload_found"], stretched), flush=True)
            with open(path, "w") as fh:                         # (after every entry: a run that is cut short leaves what it measured)
                json.dump(out, fh, indent=1)
                fh.write("\n")
        del clips
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] in ("-h", "--help"):
        sys.exit(__doc__)
    opts = {"--counts": None, "--only": "a,b,c", "--sets": "f44_tenth,f44_all,s48_tenth,s48_all"}
    for name in list(opts):
        if name in args:
            k = args.index(name)
            opts[name] = args[k + 1]
            del args[k:k + 2]
    n_max = int(args[1]) if len(args) > 1 else 1024
    path = args[0] if args else "get_batch_speed.json"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    counts = [int(v) for v in opts["--counts"].split(",")] if opts["--counts"] else sorted({min(64, n_max), n_max})
    main(path, n_max, counts, opts["--only"].split(","), opts["--sets"].split(","))
