"""Timing of the viz node's debug panel on the device (rt_viz_mosaic_u8, rt_net_execute_frames_viz).

  1. rt_viz_mosaic_u8 alone, one pair per launch, at 1257x369 from 1280x720 bgra8 frames and at 513x257 from 672x376, beside a
     device-to-device copy on the same GPU in the same process that moves the same number of bytes (the launch's frames read + disparity
     read + panel written = the copy's bytes read + written).  That copy is the floor: the kernel also unpacks bytes and runs the area
     filter.  Buffers rotate over more than the 256 MB Infinity Cache.
  2. ResNet-18 2D (synthetic weights: same kernels as the trained ones), fp32, one pair, on a stream with graph mode on:
     rt_net_execute_frames_viz against rt_net_execute_frames(RT_DISP_PIXELS_F32).  The difference should be the panel's own time; a
     larger one means a synchronisation crept in.

Device events around every timed window, warm-up first, the variants of a row alternated over several rounds; median, minimum and maximum
of the rounds are reported.

    python tools/time_viz.py [--out profiles/viz.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from redtail_amd import capi, synth  # noqa: E402
from tools.time_camera_frames import HBM_PEAK, event_time  # noqa: E402

CONFIGS = [dict(w=1257, h=369, src_w=1280, src_h=720), dict(w=513, h=257, src_w=672, src_h=376)]
ROTATE_BYTES = 320 * 2 ** 20         # more than the Infinity Cache
MAX_DISP = 96.0


def rounds_of(fns, rounds, iters, warmup):
    """{name: (median, min, max)} seconds per call; the variants alternate within every round"""
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(event_time(fn, iters, warmup))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def us(t):
    return dict(median=round(t[0] * 1e6, 2), min=round(t[1] * 1e6, 2), max=round(t[2] * 1e6, 2))


def launch_rows(k, rounds, iters, warmup):
    rows = []
    g = torch.Generator(device="cuda").manual_seed(1)
    for c in CONFIGS:
        w, h, sw, sh = c["w"], c["h"], c["src_w"], c["src_h"]
        rd, wr = 2 * sh * sw * 4 + 4 * h * w, 12 * h * w
        sets = max(3, -(-ROTATE_BYTES // (rd + wr)))
        frames = [torch.randint(0, 256, (2, 1, sh, sw * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
        disp = [torch.rand(1, 1, h, w, device="cuda", generator=g) * 110.0 - 5.0 for _ in range(sets)]
        panel = [torch.empty(1, 2 * h, 6 * w, dtype=torch.uint8, device="cuda") for _ in range(sets)]
        half = (rd + wr) // 2 // 16 * 16         # a copy of `half` bytes reads `half` and writes `half`: the launch's traffic
        a = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(sets)]
        b = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(sets)]
        it = dict(mosaic=0, copy=0, color=0)

        def nxt(key):
            it[key] = (it[key] + 1) % sets
            return it[key]

        def mosaic():
            i = nxt("mosaic")
            k.viz_mosaic_u8(frames[i][0], frames[i][1], sh, sw, sw * 4, capi.RT_ENC_BGRA8, disp[i], h, w, MAX_DISP, panel[i], 6 * w, 1)

        def copy():
            i = nxt("copy")
            b[i].copy_(a[i])

        def color():
            i = nxt("color")
            k.disparity_to_color(disp[i], 1, h, w, MAX_DISP, panel[i], 3 * w)

        t = rounds_of(dict(mosaic=mosaic, copy=copy, color=color), rounds, iters, warmup)
        row = dict(name="rt_viz_mosaic_u8", size="%dx%d" % (w, h), src="%dx%d bgra8" % (sw, sh), pairs=1, us=us(t["mosaic"]), bytes_read=rd,
                   bytes_written=wr, GBps=round((rd + wr) / t["mosaic"][0] / 1e9, 1), hbm_fraction=round((rd + wr) / t["mosaic"][0] / HBM_PEAK, 3),
                   d2d_copy_same_bytes_us=us(t["copy"]), d2d_copy_GBps=round(2 * half / t["copy"][0] / 1e9, 1),
                   mosaic_over_copy=round(t["mosaic"][0] / t["copy"][0], 2),
                   rt_disparity_to_color_us=us(t["color"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del frames, disp, panel, a, b
        torch.cuda.empty_cache()
    return rows


def net_rows(lib, rounds, iters, warmup, launches):
    rows = []
    g = torch.Generator(device="cuda").manual_seed(2)
    s = torch.cuda.Stream()
    for c, alone in zip(CONFIGS, launches):
        w, h, sw, sh = c["w"], c["h"], c["src_w"], c["src_h"]
        net = lib.create("resnet18_2D", w, h, max_batch=1, weights=synth.synth_weights_resnet18_2d())
        net.set_graph(True)
        sets = max(3, -(-ROTATE_BYTES // (2 * sh * sw * 4)))
        frames = [torch.randint(0, 256, (2, 1, sh, sw * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
        px = [torch.empty(1, 1, h, w, device="cuda") for _ in range(3)]
        panel = [torch.empty(1, 2 * h, 6 * w, dtype=torch.uint8, device="cuda") for _ in range(3)]
        it = dict(viz=0, plain=0)

        def nxt(key):
            it[key] += 1
            return it[key] % sets, it[key] % 3

        def viz():
            i, o = nxt("viz")
            net.execute_frames_viz(frames[i][0], frames[i][1], capi.RT_ENC_BGRA8, px[o], panel[o], max_disp=MAX_DISP, batch=1,
                                   stream=s.cuda_stream, src_w=sw)

        def plain():
            i, o = nxt("plain")
            net.execute_frames(frames[i][0], frames[i][1], capi.RT_ENC_BGRA8, px[o], kind=capi.RT_DISP_PIXELS_F32, batch=1,
                               stream=s.cuda_stream, src_w=sw)

        with torch.cuda.stream(s):              # events on the same stream as the work
            t = rounds_of(dict(viz=viz, plain=plain), rounds, iters, warmup)
        torch.cuda.synchronize()
        row = dict(model="resnet18_2D", size="%dx%d" % (w, h), src="%dx%d bgra8" % (sw, sh), engine="fp32", pairs=1, mode="stream+graph",
                   execute_frames_viz_us=us(t["viz"]), execute_frames_us=us(t["plain"]),
                   added_us=round((t["viz"][0] - t["plain"][0]) * 1e6, 2), mosaic_alone_us=alone["us"]["median"],
                   viz_over_plain=round(t["viz"][0] / t["plain"][0], 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
        net.destroy()
        del frames
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = capi.NetLib()
    print("backend:", lib.kernels.backend(), flush=True)
    launches = launch_rows(lib.kernels, args.rounds, args.iters, args.warmup)
    res = dict(backend=lib.kernels.backend(), hbm_peak_Bps=HBM_PEAK, rounds=args.rounds, iters=args.iters, warmup=args.warmup,
               launches=launches, net=net_rows(lib, args.rounds, max(20, args.iters // 5), args.warmup, launches))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
