"""Timing of the left-right consistency path (rt_preprocess_frames_u8_lr, rt_lr_consistency, rt_net_execute_frames_lr).

  1. The two new launches alone at 1257x369 from 1280x720 bgra8, N = 1 and 4 pairs (engine batch 2N), beside the launches they stand in
     for at the same sizes: rt_preprocess_frames_u8 at batch 2N and rt_disparity_scale on 2N maps.  Buffers rotate over more than the
     256 MB Infinity Cache.  Bytes moved = what the launch must read + write (the gather of the check re-reads cached rows: not counted);
     the HBM fraction is that over the time, against the 8.0 TB/s spec peak.
  2. ResNet-18 2D at 1257x369 (synthetic weights: same kernels as the trained ones), fp32 at N = 1 and half2 at N = 4, on a stream with
     graph mode on: rt_net_execute_frames_lr(batch N) against the same engine work done the old way, rt_net_execute_frames(batch 2N,
     RT_DISP_PIXELS_F32) on 2N frames, and against rt_net_execute_frames(batch N): what the check costs a user.
  3. The share of pixels the check keeps on the reference's sample pair (trained weights, 1025x321; fp32 and half2 engine, 1 and 3 px).

Device events around every timed window, warm-up first, the variants of a row alternated over several rounds (median reported).

    python tools/time_lr_check.py [--out profiles/lr_check.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from redtail_amd import capi, model_files, synth  # noqa: E402
from tools.time_camera_frames import HBM_PEAK, SRC_H, SRC_W, alternate  # noqa: E402

H, W = 369, 1257
ROTATE_BYTES = 320 * 2 ** 20         # more than the Infinity Cache
ACCEPT = 1.04                        # box-to-box and run-to-run spread of this machine class (profiles/README.md)


def frame_sets(pairs, g, min_sets=3):
    """enough (2, pairs, H, step) bgra8 frame batches that a launch never finds its frames in the Infinity Cache"""
    per_set = 2 * pairs * SRC_H * SRC_W * 4
    sets = max(min_sets, -(-ROTATE_BYTES // per_set))
    return [torch.randint(0, 256, (2, pairs, SRC_H, SRC_W * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]


def launch_rows(k, rounds, iters, warmup):
    rows = []
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in (1, 4):
        frames = frame_sets(2 * n, g)
        sets = len(frames)
        dst = [torch.empty(2, 2 * n, 3, H, W, device="cuda") for _ in range(sets)]
        nets = max(3, -(-ROTATE_BYTES // (2 * n * H * W * 4)))
        disp = [torch.rand(2 * n, 1, H, W, device="cuda", generator=g) * 0.1 for _ in range(nets)]
        out = [torch.empty(2 * n, 1, H, W, device="cuda") for _ in range(nets)]
        mask = [torch.empty(n, 1, H, W, dtype=torch.uint8, device="cuda") for _ in range(nets)]
        it = dict(lr=0, pair=0, check=0, scale=0)

        def nxt(key, count):
            it[key] = (it[key] + 1) % count
            return it[key]

        def lr():
            i = nxt("lr", sets)
            k.preprocess_frames_u8_lr(frames[i][0], frames[i][1], SRC_H, SRC_W, SRC_W * 4, capi.RT_ENC_BGRA8, dst[i][0], dst[i][1], H, W, n)

        def pair():
            i = nxt("pair", sets)
            k.preprocess_frames_u8(frames[i][0], frames[i][1], SRC_H, SRC_W, SRC_W * 4, capi.RT_ENC_BGRA8, dst[i][0], dst[i][1], H, W, 2 * n)

        def check():
            i = nxt("check", nets)
            k.lr_consistency(disp[i], n, H, W, float(W), 1.0, out[i], capi.RT_DISP_PIXELS_F32, mask[i])

        def scale():
            i = nxt("scale", nets)
            k.disparity_scale(disp[i], out[i], 2 * n * H * W, float(W))

        t = alternate(dict(lr=lr, pair=pair, check=check, scale=scale), rounds, iters, warmup)
        planes = 2 * 2 * n * 3 * H * W * 4
        px = n * H * W
        for name, key, rd, wr in (("rt_preprocess_frames_u8_lr (N pairs -> 2N images a side)", "lr", 2 * n * SRC_H * SRC_W * 4, planes),
                                  ("rt_preprocess_frames_u8 (2N pairs)", "pair", 2 * 2 * n * SRC_H * SRC_W * 4, planes),
                                  ("rt_lr_consistency (pixels + mask)", "check", 8 * px, 5 * px),
                                  ("rt_disparity_scale (2N maps)", "scale", 8 * px, 8 * px)):
            row = dict(name=name, size="%dx%d" % (W, H), pairs=n, engine_batch=2 * n, us=round(t[key] * 1e6, 2), bytes_read=rd,
                       bytes_written=wr, GBps=round((rd + wr) / t[key] / 1e9, 1), hbm_fraction=round((rd + wr) / t[key] / HBM_PEAK, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del frames, dst, disp, out, mask
        torch.cuda.empty_cache()
    return rows


def net_rows(lib, rounds, iters, warmup, launches):
    rows = []
    g = torch.Generator(device="cuda").manual_seed(2)
    s = torch.cuda.Stream()
    for half2, n in ((False, 1), (True, 4)):
        net = lib.create("resnet18_2D", W, H, max_batch=2 * n, weights=synth.synth_weights_resnet18_2d(), fp16_weights=half2)
        net.set_graph(True)
        frames = frame_sets(2 * n, g)
        sets = len(frames)
        px = [torch.empty(2 * n, 1, H, W, device="cuda") for _ in range(3)]
        mask = [torch.empty(n, 1, H, W, dtype=torch.uint8, device="cuda") for _ in range(3)]
        it = dict(lr=0, base=0, plain=0)

        def nxt(key):
            it[key] += 1
            return it[key] % sets, it[key] % 3

        def lr():
            i, o = nxt("lr")
            net.execute_frames_lr(frames[i][0], frames[i][1], capi.RT_ENC_BGRA8, px[o], kind=capi.RT_DISP_PIXELS_F32, mask=mask[o],
                                  max_diff_px=1.0, batch=n, stream=s.cuda_stream, src_w=SRC_W)

        def base():
            i, o = nxt("base")
            net.execute_frames(frames[i][0], frames[i][1], capi.RT_ENC_BGRA8, px[o], kind=capi.RT_DISP_PIXELS_F32, batch=2 * n,
                               stream=s.cuda_stream, src_w=SRC_W)

        def plain():
            i, o = nxt("plain")
            net.execute_frames(frames[i][0], frames[i][1], capi.RT_ENC_BGRA8, px[o], kind=capi.RT_DISP_PIXELS_F32, batch=n,
                               stream=s.cuda_stream, src_w=SRC_W)

        with torch.cuda.stream(s):              # events on the same stream as the work
            t = alternate(dict(lr=lr, base=base, plain=plain), rounds, iters, warmup)
        torch.cuda.synchronize()
        ratio = t["lr"] / t["base"]
        row = dict(model="resnet18_2D", size="%dx%d" % (W, H), src="%dx%d bgra8" % (SRC_W, SRC_H), engine="half2" if half2 else "fp32", pairs=n,
                   mode="stream+graph", execute_frames_lr_us=round(t["lr"] * 1e6, 1), execute_frames_2N_us=round(t["base"] * 1e6, 1),
                   execute_frames_N_us=round(t["plain"] * 1e6, 1), lr_over_2N=round(ratio, 4), accept_at=ACCEPT, accepted=bool(ratio <= ACCEPT),
                   lr_over_N=round(t["lr"] / t["plain"], 3))
        if ratio > ACCEPT:          # which of the two new launches costs it: each against the launch it replaces, from the rows above
            alone = {(r["name"].split(" ")[0], r["pairs"]): r["us"] for r in launches}
            row["slower_by_us"] = round((t["lr"] - t["base"]) * 1e6, 1)
            row["front_end_minus_frames_u8_2N_us"] = round(alone[("rt_preprocess_frames_u8_lr", n)] - alone[("rt_preprocess_frames_u8", n)], 2)
            row["check_minus_disparity_scale_us"] = round(alone[("rt_lr_consistency", n)] - alone[("rt_disparity_scale", n)], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        net.destroy()
        del frames
        torch.cuda.empty_cache()
    return rows


def sample_rows(lib):
    """share of consistent pixels on the reference's sample pair, trained weights"""
    from PIL import Image
    rows = []
    w, h = 1025, 321
    bgr = [np.ascontiguousarray(np.array(Image.open(model_files.sample_image(side)).convert("RGB"))[None, :, :, ::-1]) for side in ("left", "right")]
    fl, fr = (torch.from_numpy(a).cuda() for a in bgr)
    for half2 in (False, True):
        net = lib.create("resnet18_2D", w, h, max_batch=2, weights_path=model_files.weight_file("resnet18_2D", half2), fp16_weights=half2)
        for max_diff in (1.0, 3.0):
            out = torch.empty(1, 1, h, w, device="cuda")
            count = torch.zeros(1, dtype=torch.int64, device="cuda")
            net.execute_frames_lr(fl, fr, capi.RT_ENC_BGR8, out, kind=capi.RT_DISP_PIXELS_F32, valid_count=count, max_diff_px=max_diff)
            row = dict(pair="tests/golden/sample", model="resnet18_2D", size="%dx%d" % (w, h), engine="half2" if half2 else "fp32",
                       max_diff_px=max_diff, valid_share=round(count.item() / (h * w), 4))
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
    launches = launch_rows(lib.kernels, args.rounds, args.iters, args.warmup)
    res = dict(backend=lib.kernels.backend(), hbm_peak_Bps=HBM_PEAK, rounds=args.rounds, iters=args.iters, warmup=args.warmup,
               launches=launches, net=net_rows(lib, args.rounds, max(20, args.iters // 5), args.warmup, launches), sample_pair=sample_rows(lib))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
