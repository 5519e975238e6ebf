"""Timing of the rectification in front of the frame path (rt_rectify_frames_u8, rt_remap_frames_u8, rt_net_execute_frames_raw).

  1. One pair, 1280x720 bgra8 and 1242x375 bgr8, same size out, a plumb_bob rig: rt_rectify_frames_u8 (positions in registers) and
     rt_remap_frames_u8 (positions from maps made by rt_rectify_maps).  Beside each, timed in the same run: a device-to-device copy of
     exactly the bytes the launch writes, and rt_preprocess_frames_u8 on the same frames (to 1257x369 / 1025x321).
  2. ResNet-18 2D 1257x369 fp32 (synthetic weights: same kernels as the trained ones) in graph mode on a stream, one 1242x375 bgr8 pair:
     rt_net_execute_frames_raw beside rt_net_execute_frames_3d on already rectified frames, same outputs (disparity + depth + cloud).

Device events around `iters` (>= 200) launches after warm-up, the compared calls alternated inside one process, `rounds` (>= 5) repeats:
min / median / max of the repeats are recorded with every figure.  Buffers rotate over more than the 256 MB Infinity Cache.

    python tools/time_rectify.py [--out profiles/rectify.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from redtail_amd import capi, synth  # noqa: E402
from tools.time_frames_any_size import alternate, rotor  # noqa: E402

H, W, FH, FW = 369, 1257, 375, 1242
PLUMB_BOB = (-0.17, 0.026, 1e-3, -5e-4, 0.0)


def rig(k, h, w, fx):
    """a left and a right camera as a calibration would give them: a few degrees of rotation, plumb_bob, a new focal length of 0.93 fx"""
    cams = []
    for side in (1.0, -1.0):
        r = np.array([0.01, -0.02 * side, 0.005])
        t = np.linalg.norm(r)
        kx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / t
        R = np.eye(3) + np.sin(t) * kx + (1 - np.cos(t)) * (kx @ kx)
        cx, cy = (w - 1) / 2 + 1.3, (h - 1) / 2 - 0.7
        K = np.array([[fx, 0, cx], [0, 0.99 * fx, cy], [0, 0, 1]])
        P = np.zeros((3, 4))
        P[:, :3] = [[0.93 * fx, 0, cx + 0.4], [0, 0.93 * fx, cy - 0.2], [0, 0, 1]]
        D = np.array(PLUMB_BOB)
        D[0] += 0.015 * (1 - side)
        cams.append(capi.RectifyCamera.from_camera_info(K, D, R, P, lib=k))
    return cams


def op_rows(k, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(4)
    cases = dict(bgra8_1280x720=(720, 1280, 4, capi.RT_ENC_BGRA8, 369, 1257, 700.0), bgr8_1242x375=(375, 1242, 3, capi.RT_ENC_BGR8, 321, 1025, 721.5))
    fns, keep, meta = {}, [], {}
    for name, (h, w, bpp, enc, nh, nw, fx) in cases.items():
        sets = max(8, int(320e6 / (4 * h * w * bpp)) + 1)                # sources + destinations of the rotation > 256 MB
        cl, cr = rig(k, h, w, fx)
        src = [torch.randint(0, 256, (2, 1, h, w * bpp), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
        dst = [torch.empty(2, 1, h, w * bpp, dtype=torch.uint8, device="cuda") for _ in range(sets)]
        pre = [torch.empty(2, 1, 3, nh, nw, device="cuda") for _ in range(sets)]
        maps = [torch.empty(h, w, device="cuda") for _ in range(4)]
        k.rectify_maps(cl, h, w, maps[0], maps[1])
        k.rectify_maps(cr, h, w, maps[2], maps[3])
        nbytes = 2 * h * w * bpp
        keep.append((src, dst, pre, maps))
        a = (src, dst, pre, maps, h, w, bpp, enc, nh, nw, cl, cr, nbytes)
        fns["rectify_" + name] = rotor(lambda i, a=a: k.rectify_frames_u8(a[0][i][0], a[0][i][1], a[4], a[5], a[5] * a[6], a[7], a[10], a[11], a[1][i][0],
                                                                         a[1][i][1], a[4], a[5], a[5] * a[6], 1), sets)
        fns["remap_" + name] = rotor(lambda i, a=a: k.remap_frames_u8(a[0][i][0], a[0][i][1], a[4], a[5], a[5] * a[6], a[7], *a[3], a[1][i][0], a[1][i][1],
                                                                     a[4], a[5], a[5] * a[6], 1), sets)
        fns["copy_" + name] = rotor(lambda i, a=a: k.check(k.lib.rt_memcpy_d2d(a[1][i].data_ptr(), a[0][i].data_ptr(), a[12], None), "rt_memcpy_d2d"), sets)
        fns["preprocess_" + name] = rotor(lambda i, a=a: k.preprocess_frames_u8(a[0][i][0], a[0][i][1], a[4], a[5], a[5] * a[6], a[7], a[2][i][0], a[2][i][1],
                                                                               a[8], a[9], 1), sets)
        inside = []
        for mx, my in ((maps[0], maps[1]), (maps[2], maps[3])):
            inside.append(float(((mx > -1) & (mx < w) & (my > -1) & (my < h)).float().mean()))
        meta[name] = dict(bytes_written=nbytes, bytes_read_at_most=nbytes, sets=sets, inside_fraction=[round(v, 3) for v in inside],
                          preprocess_to="%dx%d" % (nw, nh))
    t = alternate(fns, rounds, iters, warmup)
    rows = []
    for name in cases:
        copy = t["copy_" + name]
        for op in ("rectify", "remap"):
            cur = t[op + "_" + name]
            row = dict(name="rt_%s_frames_u8 %s, one pair, same size out" % (op, name), launches=1, **meta[name], **cur, copy_of_bytes_written=copy,
                       over_copy=round(cur["us"] / copy["us"], 2), gbytes_per_s_written=round(meta[name]["bytes_written"] / cur["us"] / 1e3, 1),
                       preprocess_frames_u8=t["preprocess_" + name])
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def net_rows(lib, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(5)
    s = torch.cuda.Stream()
    k = lib.kernels
    net = lib.create("resnet18_2D", W, H, max_batch=1, weights=synth.synth_weights_resnet18_2d())
    net.set_graph(True)
    sets = 8
    cam = capi.StereoCamera(0.93 * 721.5, 0.93 * 721.5, (FW - 1) / 2 + 1.7, (FH - 1) / 2 - 0.9, 0.54, 0.0)
    cl, cr = rig(k, FH, FW, 721.5)
    raw = [torch.randint(0, 256, (2, 1, FH, FW * 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
    rect = [torch.empty(2, 1, FH, FW * 3, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    for i in range(sets):
        k.rectify_frames_u8(raw[i][0], raw[i][1], FH, FW, FW * 3, capi.RT_ENC_BGR8, cl, cr, rect[i][0], rect[i][1], FH, FW, FW * 3, 1)
    out_f = [torch.empty(1, 1, FH, FW, device="cuda") for _ in range(3)]
    depth = [torch.empty(1, 1, FH, FW, device="cuda") for _ in range(3)]
    cloud = [torch.empty(1, FH, FW, 4, device="cuda") for _ in range(3)]
    st = s.cuda_stream
    P = capi.RT_DISP_PIXELS_F32
    fns = dict(
        frames_raw=rotor(lambda i: net.execute_frames_raw(raw[i][0], raw[i][1], capi.RT_ENC_BGR8, cl, cr, cam, disp=out_f[i % 3], kind=P, min_depth=0.5,
                                                          max_depth=80.0, depth=depth[i % 3], points=cloud[i % 3], stream=st, src_w=FW), sets),
        frames_3d=rotor(lambda i: net.execute_frames_3d(rect[i][0], rect[i][1], capi.RT_ENC_BGR8, cam, disp=out_f[i % 3], kind=P, min_depth=0.5,
                                                        max_depth=80.0, depth=depth[i % 3], points=cloud[i % 3], stream=st, src_w=FW), sets))
    with torch.cuda.stream(s):                  # events on the same stream as the work
        t = alternate(fns, rounds, iters, warmup)
    torch.cuda.synchronize()
    net.destroy()
    row = dict(model="resnet18_2D", size="%dx%d" % (W, H), engine="fp32", mode="stream+graph", src="1242x375 bgr8", pairs=1,
               outputs="disparity fp32 + depth fp32 + organised cloud", execute_frames_raw=t["frames_raw"], execute_frames_3d=t["frames_3d"],
               added_us=round(t["frames_raw"]["us"] - t["frames_3d"]["us"], 1),
               added_percent=round(100.0 * (t["frames_raw"]["us"] / t["frames_3d"]["us"] - 1.0), 2))
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
