#!/usr/bin/env python3
"""Segments with a key each (awm_add_watermark_segments_keys_d) against the best a caller could do before it, and K16t alone.

  gpu_add_segments_keys.py [timing.json]
      1024 stereo 44.1 kHz requests of 6 s (slices of one resident buffer of uniform noise x 0.98), a distinct payload each, spread over
      1, 4, 16 and 256 keys (request i has key i mod K), zero_frames on multiples of 1024:
        keys_warm     one Context.add_watermark_segments_keys for all requests, the keys of the step before
        keys_cold     the same with K keys the context has never seen (a new set per step)
        grouped_warm  the requests grouped by key, one awm_add_watermark_segments_d per key: the host builds every key's template once and
                      the context caches it (64 templates at most: with 256 keys every call evicts one)
        grouped_cold  the same with K keys the context has never seen
        one_key       K = 1 only: awm_add_watermark_segments_d itself, for the run-to-run spread the forwarding 1-key row must sit in
      "Cold" changes the keys and keeps the context: its workspaces are grown, only the templates are new.  (A fresh context would add the
      same allocations to either side.)  Host clock around calls that end in awm_ctx_synchronize, both sides in one process.  Per repeat
      the legs run one after the other (interleaved), warm-up then timed steps; a leg's figure per repeat is the median of its steps, the
      table has the median and min - max of the repeats' figures.  The outputs of keys_warm and grouped_warm are compared bit for bit.
      After the timing, one profiled call of each side gives the time per kernel scope (awm_prof_*).
        k16t / k16    256 keys per launch: key_template_kernel (awm_debug_key_templates_d, no copy out) next to frame_mod_table_kernel
                      (a batch of 256 clips of 1024 samples with a key each), from the profiling scopes; host_template: awm_tab_frame_mod_template
                      per key on one core"""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SR = 44100
SEG = 6 * SR
N_REQ = 1024
KEY_COUNTS = [1, 4, 16, 256]


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


def main(path, n_req=N_REQ, key_counts=KEY_COUNTS, repeats=3):
    import numpy as np
    import torch
    import audiowmark_amd as awm
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    ctx = awm.Context(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    pool = ((torch.rand((n_req * SEG, 2), generator=g, device="cuda") * 2 - 1) * 0.98).contiguous()
    out_pool, loop_pool = torch.empty_like(pool), torch.empty_like(pool)
    pays = payloads(n_req)
    segs = [pool[i * SEG:(i + 1) * SEG] for i in range(n_req)]
    outs = [out_pool[i * SEG:(i + 1) * SEG] for i in range(n_req)]
    loop_outs = [loop_pool[i * SEG:(i + 1) * SEG] for i in range(n_req)]
    zfs = [(i * 37 % 4000) * 1024 for i in range(n_req)]
    fresh = [1 << 20]                                      # the next test key nobody has used

    def new_keys(k):
        fresh[0] += k
        return [awm.test_key(fresh[0] - k + j) for j in range(k)]

    def stages(fn):
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

    result = {"segment_frames": SEG, "requests": n_req, "channels": 2, "repeats": repeats, "device": torch.cuda.get_device_name(0), "rows": {}}
    for k in key_counts:
        groups = [[i for i in range(n_req) if i % k == j] for j in range(k)]
        pick = lambda v, idx: [v[i] for i in idx]

        def keys_call(keys):
            ctx.add_watermark_segments_keys([keys[i % k] for i in range(n_req)], pays, segs, zfs, outs)
            ctx.synchronize()

        def grouped_call(keys):
            for j, idx in enumerate(groups):
                ctx.add_watermark_segments(keys[j], pick(pays, idx), pick(segs, idx), pick(zfs, idx), pick(loop_outs, idx))
            ctx.synchronize()

        warm = new_keys(k)
        legs = [("keys_warm", lambda: keys_call(warm), 2, 3), ("keys_cold", lambda: keys_call(new_keys(k)), 1, 3),
                ("grouped_warm", lambda: grouped_call(warm), 2, 3), ("grouped_cold", lambda: grouped_call(new_keys(k)), 1, 3)]
        if k == 1:
            legs.append(("one_key", lambda: grouped_call(warm), 2, 3))
        figures = {name: [] for name, _, _, _ in legs}
        fused_in_use = None
        for r in range(repeats):
            for name, fn, warmup, steps in legs:
                timed(fn, warmup)
                figures[name].append(statistics.median(timed(fn, steps)))
                if name == "keys_warm":
                    fused_in_use = awm.add_segments_fused_in_use()
        keys_call(warm)
        grouped_call(warm)
        equal = all(torch.equal(a, b) for a, b in zip(outs, loop_outs))
        row = {name: leg_stats(v) for name, v in figures.items()}
        row.update(fused_in_use=fused_in_use, outputs_equal=equal, stages_keys=stages(lambda: keys_call(warm)),
                   stages_grouped=stages(lambda: grouped_call(warm)),
                   grouped_warm_over_keys_warm=row["grouped_warm"]["median_ms"] / row["keys_warm"]["median_ms"],
                   grouped_cold_over_keys_cold=row["grouped_cold"]["median_ms"] / row["keys_cold"]["median_ms"])
        result["rows"][str(k)] = row
        for name, _, _, _ in legs:
            s = row[name]
            print("keys=%3d  %-12s %10.3f ms (%.3f - %.3f)" % (k, name, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
        print("keys=%3d  grouped / keys: warm x%.2f cold x%.2f  fused in use %s  equal %s" % (
              k, row["grouped_warm_over_keys_warm"], row["grouped_cold_over_keys_cold"], fused_in_use, equal), flush=True)
        for side in ("stages_keys", "stages_grouped"):
            print("keys=%3d  %s: %s" % (k, side, ", ".join("%s %.3f ms / %d" % (n, v["ms"], v["launches"]) for n, v in row[side].items())), flush=True)
        with open(path, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    # K16t next to K16, 256 keys per launch, and the host's template builder
    del pool, out_pool, loop_pool
    keys256 = b"".join(awm.key_bytes(key) for key in new_keys(256))

    def k16t():
        for _ in range(5):
            assert lib.awm_debug_key_templates_d(ctx._h, keys256, 256, None) == 0

    clips = [torch.zeros((1024, 2), device="cuda") for _ in range(256)]

    def k16():
        for _ in range(5):
            ctx.add_watermark_batch_keys([keys256[16 * i:16 * i + 16] for i in range(256)], pays[0], clips)
        ctx.synchronize()

    k16t(), k16()
    st, sk = stages(k16t)["key_template_kernel"], stages(k16)["frame_mod_table_kernel"]
    out = np.zeros(2 * 2226 * 81, np.int16)
    t0 = time.perf_counter()
    for i in range(8):
        lib.awm_tab_frame_mod_template(keys256[16 * i:16 * i + 16], out.ctypes.data_as(C.c_void_p))
    host_ms = (time.perf_counter() - t0) * 1e3 / 8
    result["k16t"] = {"key_template_kernel_ms_per_launch_of_256": st["ms"] / st["launches"],
                      "frame_mod_table_kernel_ms_per_launch_of_256": sk["ms"] / sk["launches"], "host_template_ms_per_key": host_ms}
    print("256 keys per launch: key_template_kernel %.3f ms, frame_mod_table_kernel %.3f ms; host template %.3f ms per key on one core" % (
          st["ms"] / st["launches"], sk["ms"] / sk["launches"], host_ms), flush=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("-h", "--help"):
        sys.exit(__doc__)
    main(sys.argv[1] if len(sys.argv) > 1 else "timing.json")
