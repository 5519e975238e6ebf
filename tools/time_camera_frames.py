"""Timing of the camera-frame path (rt_preprocess_frames_u8, rt_net_execute_frames) against what a caller writes without it.

  1. rt_preprocess_frames_u8 on a pair batch of 1280x720 bgra8 frames into 1257x369 and into 513x257, batch 1 and 8, beside two
     rt_preprocess_bgr8 launches on the same pixels as dense bgr8.  Inputs and outputs rotate over enough buffer sets (> 512 MB of
     frames) that no launch finds its frames in the 256 MB Infinity Cache.  Bytes moved = frames read + fp32 planes written; the HBM
     fraction is that over the time, against the 8.0 TB/s spec peak.
  2. ResNet-18 2D at 1257x369, batch 1 (synthetic weights: same kernels as the trained ones): rt_net_execute_frames(RT_DISP_PIXELS_F32)
     against the 4-launch pipeline (rt_preprocess_bgr8 x 2 -> rt_net_execute -> rt_disparity_scale), synchronous and on a stream with
     graph mode on.

Device events around every timed window, warm-up first, the two variants of a row alternated over several rounds (median reported).

    python tools/time_camera_frames.py [--out profiles/camera_frames.json]
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

HBM_PEAK = 8.0e12          # MI355X HBM3E, spec
SRC_H, SRC_W = 720, 1280


def event_time(fn, iters, warmup):
    """mean seconds per call of fn() over `iters` calls, device events on the current stream after `warmup` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def alternate(fns, rounds, iters, warmup):
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(event_time(fn, iters, warmup))
    return {k: statistics.median(v) for k, v in times.items()}


def preprocess_rows(k, rounds, iters, warmup):
    rows = []
    g = torch.Generator(device="cuda").manual_seed(1)
    for (dh, dw) in ((369, 1257), (257, 513)):
        for n in (1, 8):
            in4 = 2 * n * SRC_H * SRC_W * 4               # both frames, bgra8
            in3 = 2 * n * SRC_H * SRC_W * 3               # the same pixels as dense bgr8
            out = 2 * n * 3 * dh * dw * 4
            sets = max(2, -(-512 * 2 ** 20 // in3))
            frames = [torch.randint(0, 256, (2, n, SRC_H, SRC_W * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
            bgr = [f.view(2, n, SRC_H, SRC_W, 4)[..., :3].contiguous() for f in frames]
            dst = [torch.empty(2, n, 3, dh, dw, device="cuda") for _ in range(sets)]
            it = {"pair": 0, "two": 0}

            def pair():
                i = it["pair"] = (it["pair"] + 1) % sets
                k.preprocess_frames_u8(frames[i][0], frames[i][1], SRC_H, SRC_W, SRC_W * 4, capi.RT_ENC_BGRA8, dst[i][0], dst[i][1], dh, dw, n)

            def two():
                i = it["two"] = (it["two"] + 1) % sets
                k.preprocess_bgr8(bgr[i][0], SRC_H, SRC_W, dst[i][0], dh, dw, n)
                k.preprocess_bgr8(bgr[i][1], SRC_H, SRC_W, dst[i][1], dh, dw, n)

            t = alternate({"pair": pair, "two": two}, rounds, iters, warmup)
            for name, sec, nbytes, what in (("rt_preprocess_frames_u8 bgra8 (1 launch)", t["pair"], in4 + out, "bgra8 pair"),
                                            ("rt_preprocess_bgr8 x 2 (dense bgr8)", t["two"], in3 + out, "bgr8 x 2")):
                row = dict(name=name, src="%dx%d" % (SRC_W, SRC_H), dst="%dx%d" % (dw, dh), batch=n, us=round(sec * 1e6, 2),
                           bytes_in=in4 if "bgra8" in what else in3, bytes_out=out, GBps=round(nbytes / sec / 1e9, 1),
                           hbm_fraction=round(nbytes / sec / HBM_PEAK, 3))
                rows.append(row)
                print(json.dumps(row), flush=True)
            del frames, bgr, dst
            torch.cuda.empty_cache()
    return rows


def net_rows(lib, rounds, iters, warmup):
    k = lib.kernels
    h, w, n = 369, 1257, 1
    net = lib.create("resnet18_2D", w, h, max_batch=n, weights=synth.synth_weights_resnet18_2d())
    g = torch.Generator(device="cuda").manual_seed(2)
    frames = torch.randint(0, 256, (2, n, SRC_H, SRC_W * 4), dtype=torch.uint8, device="cuda", generator=g)
    bgr = frames.view(2, n, SRC_H, SRC_W, 4)[..., :3].contiguous()
    il, ir = torch.empty(n, 3, h, w, device="cuda"), torch.empty(n, 3, h, w, device="cuda")
    raw, px_a, px_b = (torch.empty(n, 1, h, w, device="cuda") for _ in range(3))
    rows = []
    for mode in ("sync", "stream+graph"):
        stream = None
        if mode != "sync":
            s = torch.cuda.Stream()
            stream = s.cuda_stream
            net.set_graph(True)

        def frames_call():
            net.execute_frames(frames[0], frames[1], capi.RT_ENC_BGRA8, px_a, kind=capi.RT_DISP_PIXELS_F32, batch=n, stream=stream,
                               src_w=SRC_W)

        def manual_call():
            k.preprocess_bgr8(bgr[0], SRC_H, SRC_W, il, h, w, n, stream=stream)
            k.preprocess_bgr8(bgr[1], SRC_H, SRC_W, ir, h, w, n, stream=stream)
            net.execute(il, ir, raw, n, stream=stream)
            k.disparity_scale(raw, px_b, n * h * w, float(w), stream=stream)

        if stream is None:
            t = alternate({"frames": frames_call, "manual": manual_call}, rounds, iters, warmup)
        else:
            with torch.cuda.stream(s):              # events on the same stream as the work
                t = alternate({"frames": frames_call, "manual": manual_call}, rounds, iters, warmup)
        torch.cuda.synchronize()
        assert torch.equal(px_a, px_b), "execute_frames and the manual pipeline disagree"
        for name, sec in (("rt_net_execute_frames (bgra8 -> px)", t["frames"]),
                          ("4-launch pipeline (bgr8 x 2 -> execute -> scale)", t["manual"])):
            row = dict(name=name, model="resnet18_2D", size="%dx%d" % (w, h), src="%dx%d" % (SRC_W, SRC_H), batch=n, mode=mode,
                       us=round(sec * 1e6, 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
    net.destroy()
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
    res = dict(backend=lib.kernels.backend(), hbm_peak_Bps=HBM_PEAK, rounds=args.rounds, iters=args.iters, warmup=args.warmup,
               preprocess=preprocess_rows(lib.kernels, args.rounds, args.iters, args.warmup),
               net=net_rows(lib, args.rounds, max(20, args.iters // 5), args.warmup))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
