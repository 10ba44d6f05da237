#!/usr/bin/env python3
"""Stage 0 of one group of 64 resident stereo clips of 30 s ALONE, form by form: the cost of the one launcher
(kernels.hh launch_clip_stage) beside another build of the library, e.g. the commit before it, which had a launcher per form.

  gpu_clip_stage0.py [out.json] [--tree DIR]

Legs, each STAGE_CALLS calls of awm_debug_clip_stage_d (16-bit: awm_debug_clip_stage_rates_s16_d) per timing -- every call ends in a
synchronise --, a host clock around them, every leg warmed up first, REPEATS repeats with the legs alternating inside each repeat, reported
per call as median (min - max):

  48k_phase    64 clips at 48 kHz, the phase-per-thread form
  48k_generic  the same clips with awm_debug_set_resample_phase (0): table and window in LDS
  32k          64 clips at 32 kHz: table and window in LDS
  44k_float    64 clips at 44.1 kHz: the copy
  44k_s16      the same as 16-bit PCM: the copy that converts

--tree DIR imports the package from another checkout (default: this one).  The two builds are compared by running this tool once per
build, alternating, in processes of their own.  Also recorded: the kernels of stage 0 each leg launched, by form
(awm_debug_clip_form_launches), and a checksum of the slices, which must be equal between builds."""
import ctypes as C
import json
import os
import statistics
import sys
import time

SECONDS = 30
N_CLIPS = 64
REPEATS = 5
STAGE_CALLS = 20
LEGS = (("48k_phase", 48000, False, 1), ("48k_generic", 48000, False, 0), ("32k", 32000, False, 1), ("44k_float", 44100, False, 1),
        ("44k_s16", 44100, True, 1))


def main(path, tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import audiowmark_amd as awm
    lib = awm.lib
    ctx = awm.Context(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    clips = {}
    for rate in (48000, 32000, 44100):
        clips[rate, False] = [(torch.rand((SECONDS * rate + 17 * i, 2), generator=gen, device="cuda") * 2 - 1).contiguous() for i in range(N_CLIPS)]
    clips[44100, True] = [torch.round(c * 32767).to(torch.int16).contiguous() for c in clips[44100, False]]
    out = torch.zeros((N_CLIPS, lib.awm_debug_clip_slice_values(2)), dtype=torch.float32, device="cuda")
    ranges = np.zeros((N_CLIPS, 2), np.int64)

    def forms():
        f = (C.c_long * 3)()
        lib.awm_debug_clip_form_launches(f)
        return list(f)

    def leg(rate, s16, phase):
        src = clips[rate, s16]
        ptrs = (C.c_void_p * N_CLIPS)(*[c.data_ptr() for c in src])
        frames = (C.c_size_t * N_CLIPS)(*[c.shape[0] for c in src])
        out_p, rng_p = C.c_void_p(out.data_ptr()), ranges.ctypes.data_as(C.c_void_p)

        def run():
            lib.awm_debug_set_resample_phase(phase)
            try:
                for _ in range(STAGE_CALLS):
                    rc = (lib.awm_debug_clip_stage_rates_s16_d(ctx._h, N_CLIPS, ptrs, frames, 2, None, out_p, rng_p) if s16 else
                          lib.awm_debug_clip_stage_d(ctx._h, N_CLIPS, ptrs, frames, 2, rate, out_p, rng_p))
                    assert rc == 0, lib.awm_last_error()
            finally:
                lib.awm_debug_set_resample_phase(1)
        return run
    fns = [(name, leg(rate, s16, phase)) for name, rate, s16, phase in LEGS]
    times = {name: [] for name, _ in fns}
    launched, checksum = {}, {}
    for rep in range(-1, REPEATS):                          # -1: the warm-up of every leg
        for name, fn in fns:
            before = forms()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / STAGE_CALLS
            if rep < 0:
                launched[name] = [a - b for a, b in zip(forms(), before)]
                # (what a stage leaves out keeps the buffer's contents: only the ranges and the values inside them are the stage's own)
                checksum[name] = [int(ranges.sum()), int(out.view(torch.int32)[0, ranges[0, 0]:ranges[0, 1]].to(torch.int64).sum())]
            else:
                times[name].append(ms)
                print("repeat %d  %-12s %9.4f ms per call" % (rep, name, ms), flush=True)
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    result = {"device": torch.cuda.get_device_name(0), "tree": os.path.relpath(tree, here), "n_clips": N_CLIPS, "seconds": SECONDS, "channels": 2,
              "repeats": REPEATS, "stage_calls_per_timing": STAGE_CALLS,
              "legs": {name: {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms,
                              "form_launches_generic_phase_copy": launched[name], "checksum": checksum[name]} for name, ms in times.items()}}
    for name, s in result["legs"].items():
        print("%-12s %9.4f ms (%.4f - %.4f)  forms %s  checksum %s" % (name, s["median_ms"], s["min_ms"], s["max_ms"],
                                                                     s["form_launches_generic_phase_copy"], s["checksum"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] in ("-h", "--help"):
        sys.exit(__doc__)
    tree = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    if "--tree" in args:
        k = args.index("--tree")
        tree = args[k + 1]
        del args[k:k + 2]
    main(args[0] if args else "clip_stage0.json", tree)
