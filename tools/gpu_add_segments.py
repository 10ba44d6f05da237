#!/usr/bin/env python3
"""A batch of stream segments, each with its own offset and payload (awm_add_watermark_segments_d) against the two things it sits between.

  gpu_add_segments.py [timing.json]
      256 and 1024 stereo segments of 6 s + 2 x 3072 samples of context at 44.1 kHz (slices of one resident buffer of uniform noise
      x 0.98: every limiter block ramps), zero_frames on the 1024 grid, a distinct payload each:
        fused       one Context.add_watermark_segments
        fused_r17   the same batch 17 samples further into the stream: every segment staged (gather + scatter)
        loop        per segment awm_add_stream_create_at / input copy / push / output copy / destroy on the same context -- the only way
                    before this entry point; every payload misses the context's 64 cached tables, so each pays build_frame_mod_table
        floor       awm_add_watermark_batch_d on the same clips with ONE payload (no offsets, one cached table)
        k16p_256    K16p alone: 256 tables from the key's template (awm_debug_payload_tables_d without the copy to the host)
      Host clock around calls that end in awm_ctx_synchronize.  Per repeat the legs run one after the other, warm-up then timed steps;
      a leg's figure per repeat is the median of its steps, the table has the median and min - max of the repeats' figures.  The fused
      outputs are compared with the loop's bit for bit."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SEG = 6 * 44100 + 2 * 3072
TILE = (SEG + 1023) // 1024 + 1            # frames of 1024 samples: a segment is one tile of the stream
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


def main(path, counts=COUNTS, repeats=3):
    import torch
    import audiowmark_amd as awm
    from audiowmark_amd.binding import _hip_memcpy_dtod
    lib = awm.lib
    ctx = awm.Context(0)
    n_max = max(counts)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    pool = ((torch.rand((n_max * SEG, 2), generator=g, device="cuda") * 2 - 1) * 0.98).contiguous()
    out_pool = torch.empty_like(pool)
    loop_pool = torch.empty_like(pool)
    result = {"segment_frames": SEG, "channels": 2, "repeats": repeats, "device": torch.cuda.get_device_name(0), "rows": {}}
    for n in counts:
        pays = payloads(n)
        segs = [pool[i * SEG:(i + 1) * SEG] for i in range(n)]
        outs = [out_pool[i * SEG:(i + 1) * SEG] for i in range(n)]
        loop_outs = [loop_pool[i * SEG:(i + 1) * SEG] for i in range(n)]
        zfs = [(i * 37 % 4000) * 1024 for i in range(n)]
        zfs17 = [z + 17 for z in zfs]
        esz = 8

        def fused():
            ctx.add_watermark_segments(None, pays, segs, zfs, outs)
            ctx.synchronize()

        def fused_r17():
            ctx.add_watermark_segments(None, pays, segs, zfs17, outs)
            ctx.synchronize()

        def loop(offsets=zfs):
            done_p, done_n = (C.c_void_p * 3)(), (C.c_size_t * 3)()
            for i in range(n):
                h = C.c_void_p()
                if lib.awm_add_stream_create_at(ctx._h, bytes(16), pays[i].encode(), 2, TILE, offsets[i], C.byref(h)) != 0:
                    raise RuntimeError("awm_add_stream_create_at failed")
                try:
                    _hip_memcpy_dtod(ctx, lib.awm_add_stream_input(h), segs[i].data_ptr(), SEG * esz)
                    k = lib.awm_add_stream_push(h, SEG, 1, done_p, done_n)
                    if k < 0:
                        raise RuntimeError("awm_add_stream_push failed")
                    written = 0
                    for j in range(k):
                        _hip_memcpy_dtod(ctx, loop_outs[i].data_ptr() + written * esz, done_p[j], done_n[j] * esz)
                        written += done_n[j]
                    assert written == SEG
                finally:
                    lib.awm_add_stream_destroy(h)
            ctx.synchronize()

        def floor():
            ctx.add_watermark_batch(None, pays[0], segs, outs)
            ctx.synchronize()

        hexes256 = (C.c_char_p * 256)(*[p.encode() for p in payloads(256)])

        def k16p_256():
            if lib.awm_debug_payload_tables_d(ctx._h, bytes(16), hexes256, 256, None) != 0:
                raise RuntimeError("awm_debug_payload_tables_d failed")
            ctx.synchronize()

        legs = [("fused", fused, 2, 5), ("fused_r17", fused_r17, 2, 5), ("loop", loop, 1, 2), ("floor", floor, 2, 5), ("k16p_256", k16p_256, 2, 10)]
        figures = {name: [] for name, _, _, _ in legs}
        fused_in_use = None
        for r in range(repeats):
            for name, fn, warmup, steps in legs:
                timed(fn, warmup)
                figures[name].append(statistics.median(timed(fn, steps)))
                if name == "fused":
                    fused_in_use = awm.add_segments_fused_in_use()
        # the outputs: fused == loop at both phases (the loop's last run was at r = 0)
        fused()
        equal = all(torch.equal(a, b) for a, b in zip(outs, loop_outs))
        fused_r17()
        loop(zfs17)
        equal17 = all(torch.equal(a, b) for a, b in zip(outs, loop_outs))
        row = {name: leg_stats(v) for name, v in figures.items()}
        row.update(fused_in_use=fused_in_use, outputs_equal=equal, outputs_equal_r17=equal17,
                   loop_over_fused=row["loop"]["median_ms"] / row["fused"]["median_ms"],
                   fused_over_floor=row["fused"]["median_ms"] / row["floor"]["median_ms"],
                   staging_ms=row["fused_r17"]["median_ms"] - row["fused"]["median_ms"],
                   fused_ms_per_segment=row["fused"]["median_ms"] / n, loop_ms_per_segment=row["loop"]["median_ms"] / n)
        result["rows"][str(n)] = row
        for name, _, _, _ in legs:
            s = row[name]
            print("n=%4d  %-10s %10.3f ms (%.3f - %.3f)" % (n, name, s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
        print("n=%4d  loop / fused x%.2f  fused / floor x%.2f  staging %+.3f ms  fused in use %s  equal %s / %s" % (
              n, row["loop_over_fused"], row["fused_over_floor"], row["staging_ms"], fused_in_use, equal, equal17), flush=True)
        with open(path, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("-h", "--help"):
        sys.exit(__doc__)
    main(sys.argv[1] if len(sys.argv) > 1 else "timing.json")
