#!/usr/bin/env python3
"""BASELINE configs[4] at 48 kHz: `get` of 1024 resident stereo clips of 30 s, marked at 48 kHz.

  gpu_get_batch_rate.py [out.json] [n_clips]

Legs, each a host clock around a call that ends in a synchronise, every leg warmed up first, REPEATS repeats with the legs alternating
inside each repeat, reported as median (min - max):

  a       awm_get_watermark_batch_rate_d on the 48 kHz clips (short clips: K10c straight into the groups' padded slices)
  b       what the tree offered before: a loop of awm_resample_d into n_clips buffers, then awm_get_watermark_batch_d on them
  c       the floor: awm_get_watermark_batch_d on clips resampled beforehand
  a_keys  a with a key per clip (clips marked with their keys), awm_get_watermark_batch_keys_rate_d
  b_keys  b with a key per clip
  stage_phase / stage_generic
          stage 0 alone (awm_debug_clip_stage_d, 64 clips, STAGE_CALLS calls per timing) with the phase form of K10c and under
          awm_debug_set_resample_phase (0)

Also: the results of a, b and c compared (they must be equal), device bytes each leg needs beyond its inputs (computed from the shapes:
the 44.1 kHz copies), and the scope clip_resample_pad_kernel of one further run of a: launches, milliseconds, algorithmic bytes and
their share of the peak HBM bandwidth (a figure of the scope between its events on a lane's stream, beside the other lanes' work; which
resource bounds the kernel is worked out from the shapes in DESIGN.md section 10)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

RATE = 48000
SECONDS = 30
REPEATS = 3
STAGE_CALLS = 20
HBM_PEAK = 8.0e12            # bytes / s, specification (6.29e12 measured with a float4 copy)
PAY1 = "0123456789abcdef0011223344556677"
PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def main(path, n_clips):
    import torch
    import audiowmark_amd as awm
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    ctx = awm.Context(0)
    n = SECONDS * RATE
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    keys = [awm.test_key(1 + i) for i in range(n_clips)]

    def marked(per_clip_key):
        out = []
        for i in range(n_clips):
            x = (torch.rand((n, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
            out.append(ctx.add_watermark(keys[i] if per_clip_key else None, PAY1 if i % 2 else PAY2, x, sample_rate=RATE))
        ctx.synchronize()
        return out
    clips, clips_k = marked(False), marked(True)
    n44 = ctx.resample_frames(n, RATE, 44100)
    copies = [torch.empty((n44, 2), dtype=torch.float32, device="cuda") for _ in range(n_clips)]

    def resample_all(src):
        for s, d in zip(src, copies):
            ctx.resample(s, RATE, 44100, out=d)

    results = {}

    def leg_a():
        results["a"] = ctx.get_watermark_batch(None, clips, sample_rate=RATE)

    def leg_b():
        resample_all(clips)
        results["b"] = ctx.get_watermark_batch(None, copies)

    def leg_a_keys():
        results["a_keys"] = ctx.get_watermark_batch_keys(keys, clips_k, sample_rate=RATE)

    def leg_b_keys():
        resample_all(clips_k)
        results["b_keys"] = ctx.get_watermark_batch_keys(keys, copies)

    def leg_c():
        results["c"] = ctx.get_watermark_batch(None, copies)

    def prepare_c():
        resample_all(clips)
        ctx.synchronize()

    stage_clips = clips[:64]
    stage_buf = torch.zeros((len(stage_clips), lib.awm_debug_clip_slice_values(2)), dtype=torch.float32, device="cuda")

    def stage(phase):
        def run():
            lib.awm_debug_set_resample_phase(phase)
            try:
                for _ in range(STAGE_CALLS):
                    ctx.clip_stage(stage_clips, RATE, out=stage_buf)
            finally:
                lib.awm_debug_set_resample_phase(1)
        return run

    # (leg c reads the copies of the one-key clips: they are restored, untimed, in front of it)
    legs = [("a", leg_a, None), ("b", leg_b, None), ("a_keys", leg_a_keys, None), ("b_keys", leg_b_keys, None), ("c", leg_c, prepare_c),
            ("stage_phase", stage(1), None), ("stage_generic", stage(0), None)]
    times = {name: [] for name, _, _ in legs}
    for rep in range(-1, REPEATS):                          # -1: the warm-up of every leg
        for name, fn, before in legs:
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if rep >= 0:
                times[name].append(ms / (STAGE_CALLS if name.startswith("stage") else 1))
                print("repeat %d  %-13s %9.3f ms" % (rep, name, times[name][-1]), flush=True)

    # the scope of K10c in one further run of a
    ctx.synchronize()
    lib.awm_prof_enable(ctx._h, 1)
    prof = {}
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
    k = prof.get("clip_resample_pad_kernel")
    if k and k["ms"] > 0:
        k["bytes_per_s"] = k["algorithmic_bytes"] / (k["ms"] * 1e-3)
        k["share_of_hbm_peak"] = k["bytes_per_s"] / HBM_PEAK

    copy_bytes = n_clips * n44 * 2 * 4
    found = sum(any(p["bits"] == (PAY1 if i % 2 else PAY2) for p in r) for i, r in enumerate(results["a"]))
    out = {"device": torch.cuda.get_device_name(0), "n_clips": n_clips, "seconds": SECONDS, "rate": RATE, "channels": 2, "repeats": REPEATS,
           "stage_clips": len(stage_clips), "stage_calls_per_timing": STAGE_CALLS,
           "legs": {name: summary(ms) for name, ms in times.items()},
           "equal": {"a_b": results["a"] == results["b"], "a_c": results["a"] == results["c"], "a_keys_b_keys": results["a_keys"] == results["b_keys"]},
           "payloads_found_a": found,
           "payloads_found_a_keys": sum(any(p["bits"] == (PAY1 if i % 2 else PAY2) for p in r) for i, r in enumerate(results["a_keys"])),
           "extra_device_bytes": {"a": 0, "a_keys": 0, "b": copy_bytes, "b_keys": copy_bytes, "c": copy_bytes,
                                  "note": "beyond the inputs and the lanes' group workspaces, which every leg has alike: the 44.1 kHz copies"},
           "prof_a": prof}
    for name, s in out["legs"].items():
        print("%-13s %9.3f ms (%.3f - %.3f)" % (name, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
    print("equal:", out["equal"], " payloads found:", found, "of", n_clips, flush=True)
    print("clip_resample_pad_kernel:", k, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("-h", "--help"):
        sys.exit(__doc__)
    main(sys.argv[1] if len(sys.argv) > 1 else "get_batch_rate.json", int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
