"""Timing of the depth / point-cloud path (rt_disparity_to_points, rt_net_execute_frames_3d).

  1. rt_disparity_to_points 1257x369 -> 1242x375 with a left-right mask off: (a) depth only, (b) organised cloud with bgr8 colour,
     (c) depth + cloud + disparity, (d) compact cloud + count.  Beside each row, timed in the same run: a device-to-device copy of exactly
     the bytes the row writes, and the unchanged rt_disparity_to_frame (fp32).  Target for (a)-(c): one launch that costs no more than
     rt_disparity_to_frame plus the copy time of the additional bytes written, the margin being the [min, max] spread of the windows.
  2. ResNet-18 2D 1257x369 fp32 (synthetic weights: same kernels as the trained ones) in graph mode on a stream, one 1242x375 bgr8 pair:
     rt_net_execute_frames_3d (disparity + depth + organised cloud) beside rt_net_execute_frames_ex on the same arguments.

Device events around `iters` (>= 200) launches after warm-up, the compared calls alternated inside one process, `rounds` (>= 5) repeats:
min / median / max of the repeats are recorded with every figure.  Buffers rotate over more than the 256 MB Infinity Cache.

    python tools/time_points.py [--out profiles/points.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from redtail_amd import capi, synth  # noqa: E402
from tools.time_frames_any_size import alternate, rotor  # noqa: E402

SETS = 24                    # rotation: 24 x (7.5 MB cloud + 1.9 MB maps + sources) > 256 MB
H, W, FH, FW = 369, 1257, 375, 1242
KITTI = dict(fx=721.5377, fy=721.5377, cx=609.5593, cy=172.854, baseline=0.54, doffs=0.0)


def op_rows(k, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(2)
    cam = capi.StereoCamera(*KITTI.values())
    plane = FH * FW
    px = [torch.rand(1, 1, H, W, device="cuda", generator=g) * 90 + 3 for _ in range(SETS)]
    left = [torch.randint(0, 256, (1, FH, FW * 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(SETS)]
    disp = [torch.empty(1, 1, FH, FW, device="cuda") for _ in range(SETS)]
    depth = [torch.empty(1, 1, FH, FW, device="cuda") for _ in range(SETS)]
    cloud = [torch.empty(1, FH, FW, 4, device="cuda") for _ in range(SETS)]
    src = [torch.rand(plane * 6, device="cuda", generator=g) for _ in range(SETS)]          # 24 bytes a pixel: the largest row
    dst = [torch.empty(plane * 6, device="cuda") for _ in range(SETS)]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(k.points_workspace_bytes(1, FH, FW), dtype=torch.uint8, device="cuda")
    BGR = capi.RT_ENC_BGR8
    rows = dict(
        a_depth=(4 * plane, 1, lambda i: k.disparity_to_points(px[i], 1, H, W, FH, FW, cam, 0.5, 80.0, depth=depth[i])),
        b_cloud_bgr8=(16 * plane, 1, lambda i: k.disparity_to_points(px[i], 1, H, W, FH, FW, cam, 0.5, 80.0, color=left[i], encoding=BGR,
                                                                    points=cloud[i])),
        c_depth_cloud_disparity=(24 * plane, 1, lambda i: k.disparity_to_points(px[i], 1, H, W, FH, FW, cam, 0.5, 80.0, color=left[i], encoding=BGR,
                                                                               disp_out=disp[i], depth=depth[i], points=cloud[i])),
        d_compact_cloud_count=(16 * plane, 2, lambda i: k.disparity_to_points(px[i], 1, H, W, FH, FW, cam, 0.5, 80.0, color=left[i], encoding=BGR,
                                                                             points_compact=cloud[i], count=cnt, workspace=ws)))
    fns = {name: rotor(fn, SETS) for name, (_, _, fn) in rows.items()}
    fns["to_frame_fp32"] = rotor(lambda i: k.disparity_to_frame(px[i], 1, H, W, disp[i], FH, FW, kind=capi.RT_DISP_PIXELS_F32), SETS)
    for nbytes in sorted({b for b, _, _ in rows.values()} | {4 * plane, 12 * plane, 20 * plane}):
        fns["copy_%d" % nbytes] = rotor(lambda i, nb=nbytes: k.check(k.lib.rt_memcpy_d2d(dst[i].data_ptr(), src[i].data_ptr(), nb, None), "rt_memcpy_d2d"), SETS)
    t = alternate(fns, rounds, iters, warmup)
    base = t["to_frame_fp32"]
    out = []
    for name, (nbytes, launches, _) in rows.items():
        extra = nbytes - 4 * plane                       # bytes written beyond rt_disparity_to_frame's fp32 map
        extra_copy = t["copy_%d" % extra]["us"] if extra else 0.0
        spread = t[name]["max_us"] - t[name]["min_us"]
        target = base["us"] + extra_copy
        row = dict(name="rt_disparity_to_points 1257x369 -> 1242x375 " + name, launches=launches, out_bytes=nbytes, **t[name],
                   copy_of_out_bytes=t["copy_%d" % nbytes], disparity_to_frame_fp32=base, extra_bytes=extra, copy_of_extra_bytes_us=extra_copy,
                   target_us=round(target, 2), over_target_us=round(t[name]["us"] - target, 2), spread_us=round(spread, 2),
                   meets_target=bool(launches == 1 and t[name]["us"] - target <= spread))
        out.append(row)
        print(json.dumps(row), flush=True)
    out[3]["over_b"] = round(t["d_compact_cloud_count"]["us"] / t["b_cloud_bgr8"]["us"], 2)
    out[3].pop("meets_target")
    cnt_host = int(cnt.cpu()[0])
    out[3]["valid_fraction"] = round(cnt_host / plane, 3)
    return out


def net_rows(lib, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(3)
    s = torch.cuda.Stream()
    net = lib.create("resnet18_2D", W, H, max_batch=1, weights=synth.synth_weights_resnet18_2d())
    net.set_graph(True)
    sets = 8
    cam = capi.StereoCamera(*KITTI.values())
    kitti = [torch.randint(0, 256, (2, 1, FH, FW * 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
    out_f = [torch.empty(1, 1, FH, FW, device="cuda") for _ in range(3)]
    depth = [torch.empty(1, 1, FH, FW, device="cuda") for _ in range(3)]
    cloud = [torch.empty(1, FH, FW, 4, device="cuda") for _ in range(3)]
    st = s.cuda_stream
    P = capi.RT_DISP_PIXELS_F32
    fns = dict(
        frames_3d=rotor(lambda i: net.execute_frames_3d(kitti[i][0], kitti[i][1], capi.RT_ENC_BGR8, cam, disp=out_f[i % 3], kind=P, min_depth=0.5,
                                                        max_depth=80.0, depth=depth[i % 3], points=cloud[i % 3], stream=st, src_w=FW), sets),
        frames_ex=rotor(lambda i: net.execute_frames_ex(kitti[i][0], kitti[i][1], capi.RT_ENC_BGR8, out_f[i % 3], kind=P, stream=st, src_w=FW), sets))
    with torch.cuda.stream(s):                  # events on the same stream as the work
        t = alternate(fns, rounds, iters, warmup)
    torch.cuda.synchronize()
    net.destroy()
    row = dict(model="resnet18_2D", size="%dx%d" % (W, H), engine="fp32", mode="stream+graph", src="1242x375 bgr8", pairs=1,
               execute_frames_3d=dict(outputs="disparity fp32 + depth fp32 + organised cloud", **t["frames_3d"]),
               execute_frames_ex=dict(outputs="disparity fp32", **t["frames_ex"]), added_us=round(t["frames_3d"]["us"] - t["frames_ex"]["us"], 1),
               added_percent=round(100.0 * (t["frames_3d"]["us"] / t["frames_ex"]["us"] - 1.0), 2))
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = capi.NetLib()
    print("backend:", lib.kernels.backend(), flush=True)
    res = dict(backend=lib.kernels.backend(), rounds=args.rounds, iters=args.iters, warmup=args.warmup,
               note="us = median of `rounds` windows of `iters` launches between device events; min_us / max_us = their spread",
               op=op_rows(lib.kernels, args.rounds, args.iters, args.warmup), net=net_rows(lib, args.rounds, args.iters, args.warmup))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
