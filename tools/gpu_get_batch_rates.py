#!/usr/bin/env python3
"""`get` of N resident stereo clips of 30 s whose sample rates are MIXED: the rate of clip i is drawn with a fixed
seed from 44.1, 48, 32, 96, 22.05 and 88.2 kHz, and every clip is marked at its rate.

  gpu_get_batch_rates.py [out.json] [n_clips] [--legs a,b,...] [--tree DIR]

Legs, each a host clock around calls that end in a synchronise, every leg warmed up first, REPEATS repeats with the legs alternating
inside each repeat, reported as median (min - max):

  a        awm_get_watermark_batch_rates_d: one call, the groups of 64 fill in call order whatever the rates
  b        what a caller did before: the clips sorted by rate, one awm_get_watermark_batch_rate_d call per rate (44.1 kHz:
           awm_get_watermark_batch_d)
  a_keys   a with a key per clip (clips marked with their keys), awm_get_watermark_batch_keys_rates_d
  b_keys   b with a key per clip
  c_new    N clips that are ALL at 48 kHz through awm_get_watermark_batch_rates_d (it forwards) ...
  c_old    ... and through awm_get_watermark_batch_rate_d
  stage_mixed / stage_48k
           stage 0 alone, STAGE_CALLS calls per timing: one mixed group of 64 (awm_debug_clip_stage_rates_d, K10x) beside the one-rate stage
           of 64 clips at 48 kHz (awm_debug_clip_stage_d, K10c)

--legs runs a subset (b and b_keys need nothing of this tree's new entry points); --tree DIR imports the package from another checkout,
e.g. a build of the parent commit, so that b can be timed there on the same material.

Also: a and b compared clip by clip (they must be equal), the payloads found, the clips per rate, and the profiling scopes of one further
run of a: launches, milliseconds and algorithmic bytes of clip_stage_mixed_kernel."""
import ctypes as C
import json
import os
import statistics
import sys
import time

RATES = (44100, 48000, 32000, 96000, 22050, 88200)
SECONDS = 30
REPEATS = 3
STAGE_CALLS = 20
SEED = 20240611
PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"
ALL_LEGS = ("a", "b", "a_keys", "b_keys", "c_new", "c_old", "stage_mixed", "stage_48k")


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def main(path, n_clips, want_legs, tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import audiowmark_amd as awm
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    ctx = awm.Context(0)
    rates = [RATES[k] for k in np.random.default_rng(SEED).integers(0, len(RATES), n_clips)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    keys = [awm.test_key(1 + i) for i in range(n_clips)]

    def marked(clip_rates, per_clip_key):
        out = []
        for i, r in enumerate(clip_rates):
            x = (torch.rand((SECONDS * r, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
            out.append(ctx.add_watermark(keys[i] if per_clip_key else None, PAY1 if i % 2 else PAY2, x, sample_rate=r))
        ctx.synchronize()
        return out
    need = lambda *names: any(n in want_legs for n in names)           # noqa: E731
    clips = marked(rates, False) if need("a", "b", "stage_mixed") else []
    clips_k = marked(rates, True) if need("a_keys", "b_keys") else []
    clips_48 = marked([48000] * n_clips, False) if need("c_new", "c_old", "stage_48k") else []
    by_rate = {r: [i for i in range(n_clips) if rates[i] == r] for r in RATES}
    results = {}

    def sorted_calls(call, src):
        out = [None] * n_clips
        for r, idx in by_rate.items():
            if idx:
                for i, res in zip(idx, call(r, idx, [src[i] for i in idx])):
                    out[i] = res
        return out

    def leg_a():
        results["a"] = ctx.get_watermark_batch(None, clips, sample_rate=rates)

    def leg_b():
        results["b"] = sorted_calls(lambda r, idx, sub: ctx.get_watermark_batch(None, sub, sample_rate=r), clips)

    def leg_a_keys():
        results["a_keys"] = ctx.get_watermark_batch_keys(keys, clips_k, sample_rate=rates)

    def leg_b_keys():
        results["b_keys"] = sorted_calls(lambda r, idx, sub: ctx.get_watermark_batch_keys([keys[i] for i in idx], sub, sample_rate=r), clips_k)

    def leg_c_new():
        results["c_new"] = ctx.get_watermark_batch(None, clips_48, sample_rate=[48000] * n_clips)

    def leg_c_old():
        results["c_old"] = ctx.get_watermark_batch(None, clips_48, sample_rate=48000)

    stage_buf = torch.zeros((64, lib.awm_debug_clip_slice_values(2)), dtype=torch.float32, device="cuda")

    def leg_stage_mixed():
        for _ in range(STAGE_CALLS):
            ctx.clip_stage(clips[:64], rates[:64], out=stage_buf)

    def leg_stage_48k():
        for _ in range(STAGE_CALLS):
            ctx.clip_stage(clips_48[:64], 48000, out=stage_buf)

    fns = {"a": leg_a, "b": leg_b, "a_keys": leg_a_keys, "b_keys": leg_b_keys, "c_new": leg_c_new, "c_old": leg_c_old,
           "stage_mixed": leg_stage_mixed, "stage_48k": leg_stage_48k}
    legs = [(name, fns[name]) for name in ALL_LEGS if name in want_legs and (n_clips >= 64 or not name.startswith("stage"))]
    times = {name: [] for name, _ in legs}
    for rep in range(-1, REPEATS):                          # -1: the warm-up of every leg
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if rep >= 0:
                times[name].append(ms / (STAGE_CALLS if name.startswith("stage") else 1))
                print("repeat %d  %-12s %9.3f ms" % (rep, name, times[name][-1]), flush=True)

    prof = {}
    if "a" in want_legs:                                    # the scopes of one further run of a
        ctx.synchronize()
        lib.awm_prof_enable(ctx._h, 1)
        try:
            lib.awm_prof_reset(ctx._h)
            leg_a()
            ctx.synchronize()
            for i in range(lib.awm_prof_count()):
                ms, launches, nbytes = C.c_double(), C.c_long(), C.c_double()
                lib.awm_prof_read(ctx._h, i, C.byref(ms), C.byref(launches), C.byref(nbytes))
                if launches.value:
                    prof[lib.awm_prof_name(i).decode()] = {"launches": launches.value, "ms": ms.value, "algorithmic_bytes": nbytes.value}
        finally:
            lib.awm_prof_enable(ctx._h, 0)

    def found(name):
        return sum(any(p["bits"] == (PAY1 if i % 2 else PAY2) for p in r) for i, r in enumerate(results[name])) if name in results else None
    equal = {}
    for x, y in (("a", "b"), ("a_keys", "b_keys"), ("c_new", "c_old")):
        if x in results and y in results:
            equal[x + "_" + y] = results[x] == results[y]
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    out = {"device": torch.cuda.get_device_name(0), "tree": os.path.relpath(tree, here), "n_clips": n_clips, "seconds": SECONDS, "channels": 2,
           "repeats": REPEATS, "seed": SEED, "clips_per_rate": {str(r): len(idx) for r, idx in by_rate.items()},
           "groups_of_64": {"a": (n_clips + 63) // 64, "b": sum((len(idx) + 63) // 64 for idx in by_rate.values())},
           "stage_calls_per_timing": STAGE_CALLS, "legs": {name: summary(ms) for name, ms in times.items()}, "equal": equal,
           "payloads_found": {name: found(name) for name in ("a", "b", "a_keys", "b_keys", "c_new", "c_old") if name in results},
           "prof_a": prof}
    for name, s in out["legs"].items():
        print("%-12s %9.3f ms (%.3f - %.3f)" % (name, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
    print("equal:", equal, " payloads found:", out["payloads_found"], "of", n_clips, " clips per rate:", out["clips_per_rate"], flush=True)
    print("clip_stage_mixed_kernel:", prof.get("clip_stage_mixed_kernel"), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] in ("-h", "--help"):
        sys.exit(__doc__)
    legs, tree = ALL_LEGS, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    for flag in ("--legs", "--tree"):
        if flag in args:
            k = args.index(flag)
            value = args[k + 1]
            del args[k:k + 2]
            if flag == "--legs":
                legs = tuple(value.split(","))
            else:
                tree = value
    main(args[0] if args else "get_batch_rates.json", int(args[1]) if len(args) > 1 else 1024, legs, tree)
