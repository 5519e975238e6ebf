"""Timing of the any-size frame path (rt_preprocess_frames_u8_cv, rt_disparity_to_frame, rt_net_execute_frames_ex).

  1. rt_preprocess_frames_u8_cv 1242x375 bgr8 -> 1257x369 and 672x376 bgra8 -> 1025x321, beside rt_preprocess_frames_u8 1280x720 bgra8 ->
     1257x369 (the yardstick: unchanged kernel, 17.7 us in profiles/camera_frames.json) in the same process.
  2. rt_disparity_to_frame 1257x369 -> 1242x375, fp32 and 16-bit, with and without mask (and its count), beside a device-to-device copy of the output bytes.
  3. ResNet-18 2D 1257x369 fp32 (synthetic weights: same kernels as the trained ones) in graph mode on a stream:
     rt_net_execute_frames_ex (RT_RESIZE_CV_AREA, RT_GEOM_FRAME, without / with a check) from 1242x375 bgr8 beside rt_net_execute_frames /
     rt_net_execute_frames_lr from 1280x720 bgra8: the added time per pair.

Device events around `iters` (>= 200) launches after warm-up, the compared calls alternated inside one process, `rounds` (>= 5) repeats:
min / median / max of the repeats are recorded with every figure.  Buffers rotate over more than the 256 MB Infinity Cache.

    python tools/time_frames_any_size.py [--out profiles/frames_any_size.json]
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
from tools.time_camera_frames import event_time  # noqa: E402

SETS = 24                    # rotation: 24 x 11 MB of planes / 24 x 1.9 MB of maps plus their sources


def alternate(fns, rounds, iters, warmup):
    """{name: dict(us=median, min_us=, max_us=)} of `rounds` timed windows per function, the functions taking turns"""
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(event_time(fn, iters, warmup) * 1e6)
    return {k: dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in times.items()}


def rotor(fn, count):
    state = [0]

    def call():
        state[0] = (state[0] + 1) % count
        fn(state[0])
    return call


def front_rows(k, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(1)
    cases = dict(cv_1242x375_bgr8_to_1257x369=(375, 1242, 3, capi.RT_ENC_BGR8, 369, 1257, True),
                 cv_672x376_bgra8_to_1025x321=(376, 672, 4, capi.RT_ENC_BGRA8, 321, 1025, True),
                 frames_u8_1280x720_bgra8_to_1257x369=(720, 1280, 4, capi.RT_ENC_BGRA8, 369, 1257, False))
    fns, keep = {}, []
    for name, (sh, sw, bpp, enc, dh, dw, cv) in cases.items():
        src = [torch.randint(0, 256, (2, 1, sh, sw * bpp), dtype=torch.uint8, device="cuda", generator=g) for _ in range(SETS)]
        dst = [torch.empty(2, 1, 3, dh, dw, device="cuda") for _ in range(SETS)]
        keep.append((src, dst))
        if cv:
            fns[name] = rotor(lambda i, a=(src, dst, sh, sw, bpp, enc, dh, dw): k.preprocess_frames_u8_cv(
                a[0][i][0], a[0][i][1], a[2], a[3], a[3] * a[4], a[5], a[1][i][0], a[1][i][1], a[6], a[7], 1), SETS)
        else:
            fns[name] = rotor(lambda i, a=(src, dst, sh, sw, bpp, enc, dh, dw): k.preprocess_frames_u8(
                a[0][i][0], a[0][i][1], a[2], a[3], a[3] * a[4], a[5], a[1][i][0], a[1][i][1], a[6], a[7], 1), SETS)
    t = alternate(fns, rounds, iters, warmup)
    rows = []
    yard = t["frames_u8_1280x720_bgra8_to_1257x369"]
    for name, (sh, sw, bpp, enc, dh, dw, cv) in cases.items():
        row = dict(name=("rt_preprocess_frames_u8_cv " if cv else "rt_preprocess_frames_u8 ") + name, pairs=1, bytes_read=2 * sh * sw * bpp,
                   bytes_written=2 * 3 * dh * dw * 4, **t[name])
        if cv:
            row["over_yardstick"] = round(t[name]["us"] / yard["us"], 3)
            row["yardstick_spread_us"] = round(yard["max_us"] - yard["min_us"], 2)
            row["slower_than_yardstick_beyond_spread"] = bool(t[name]["us"] - yard["us"] > yard["max_us"] - yard["min_us"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def back_rows(k, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(2)
    H, W, fh, fw = 369, 1257, 375, 1242
    px = [torch.rand(1, 1, H, W, device="cuda", generator=g) * 190 for _ in range(SETS)]
    mask = [(torch.rand(1, 1, H, W, device="cuda", generator=g) > 0.1).to(torch.uint8) * 255 for _ in range(SETS)]
    out32 = [torch.empty(1, 1, fh, fw, device="cuda") for _ in range(SETS)]
    out16 = [torch.empty(1, 1, fh, fw, dtype=torch.int16, device="cuda") for _ in range(SETS)]
    om = [torch.empty(1, 1, fh, fw, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    src32 = [torch.rand(1, 1, fh, fw, device="cuda", generator=g) for _ in range(SETS)]
    fns = dict(
        fp32=rotor(lambda i: k.disparity_to_frame(px[i], 1, H, W, out32[i], fh, fw, kind=capi.RT_DISP_PIXELS_F32), SETS),
        u16=rotor(lambda i: k.disparity_to_frame(px[i], 1, H, W, out16[i], fh, fw, kind=capi.RT_DISP_KITTI_U16), SETS),
        fp32_mask=rotor(lambda i: k.disparity_to_frame(px[i], 1, H, W, out32[i], fh, fw, kind=capi.RT_DISP_PIXELS_F32, mask=mask[i], out_mask=om[i],
                                                       valid_count=cnt), SETS),
        fp32_mask_no_count=rotor(lambda i: k.disparity_to_frame(px[i], 1, H, W, out32[i], fh, fw, kind=capi.RT_DISP_PIXELS_F32, mask=mask[i],
                                                                out_mask=om[i]), SETS),
        u16_mask=rotor(lambda i: k.disparity_to_frame(px[i], 1, H, W, out16[i], fh, fw, kind=capi.RT_DISP_KITTI_U16, mask=mask[i], out_mask=om[i],
                                                      valid_count=cnt), SETS),
        copy_fp32_bytes=rotor(lambda i: k.check(k.lib.rt_memcpy_d2d(out32[i].data_ptr(), src32[i].data_ptr(), fh * fw * 4, None), "rt_memcpy_d2d"), SETS),
        copy_u16_bytes=rotor(lambda i: k.check(k.lib.rt_memcpy_d2d(out16[i].data_ptr(), src32[i].data_ptr(), fh * fw * 2, None), "rt_memcpy_d2d"), SETS))
    t = alternate(fns, rounds, iters, warmup)
    rows = []
    for name in ("fp32", "u16", "fp32_mask_no_count", "fp32_mask", "u16_mask"):
        copy = t["copy_u16_bytes" if name.startswith("u16") else "copy_fp32_bytes"]
        row = dict(name="rt_disparity_to_frame 1257x369 -> 1242x375 " + name, out_bytes=fh * fw * (2 if name.startswith("u16") else 4), **t[name],
                   copy_us=copy["us"], copy_min_us=copy["min_us"], copy_max_us=copy["max_us"], over_copy=round(t[name]["us"] / copy["us"], 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def net_rows(lib, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(3)
    H, W = 369, 1257
    s = torch.cuda.Stream()
    net = lib.create("resnet18_2D", W, H, max_batch=2, weights=synth.synth_weights_resnet18_2d())
    net.set_graph(True)
    sets = 8
    kitti = [torch.randint(0, 256, (2, 1, 375, 1242 * 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
    hd = [torch.randint(0, 256, (2, 1, 720, 1280 * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
    out_f = [torch.empty(1, 1, 375, 1242, device="cuda") for _ in range(3)]
    out_n = [torch.empty(1, 1, H, W, device="cuda") for _ in range(3)]
    mask_f = [torch.empty(1, 1, 375, 1242, dtype=torch.uint8, device="cuda") for _ in range(3)]
    mask_n = [torch.empty(1, 1, H, W, dtype=torch.uint8, device="cuda") for _ in range(3)]
    st = s.cuda_stream
    P = capi.RT_DISP_PIXELS_F32
    fns = dict(
        ex_frame=rotor(lambda i: net.execute_frames_ex(kitti[i][0], kitti[i][1], capi.RT_ENC_BGR8, out_f[i % 3], kind=P, stream=st, src_w=1242), sets),
        frames=rotor(lambda i: net.execute_frames(hd[i][0], hd[i][1], capi.RT_ENC_BGRA8, out_n[i % 3], kind=P, stream=st, src_w=1280), sets),
        ex_frame_check=rotor(lambda i: net.execute_frames_ex(kitti[i][0], kitti[i][1], capi.RT_ENC_BGR8, out_f[i % 3], kind=P, max_diff_px=1.0,
                                                             mask=mask_f[i % 3], stream=st, src_w=1242), sets),
        frames_lr=rotor(lambda i: net.execute_frames_lr(hd[i][0], hd[i][1], capi.RT_ENC_BGRA8, out_n[i % 3], kind=P, mask=mask_n[i % 3],
                                                        max_diff_px=1.0, stream=st, src_w=1280), sets))
    with torch.cuda.stream(s):                  # events on the same stream as the work
        t = alternate(fns, rounds, iters, warmup)
    torch.cuda.synchronize()
    net.destroy()
    rows = []
    for new, old, what in (("ex_frame", "frames", "no check"), ("ex_frame_check", "frames_lr", "check at 1 px")):
        row = dict(model="resnet18_2D", size="%dx%d" % (W, H), engine="fp32", mode="stream+graph", what=what,
                   execute_frames_ex=dict(src="1242x375 bgr8", resize="RT_RESIZE_CV_AREA", geometry="RT_GEOM_FRAME", **t[new]),
                   existing_call=dict(name="rt_net_execute_frames" + ("_lr" if old == "frames_lr" else ""), src="1280x720 bgra8", **t[old]),
                   added_us=round(t[new]["us"] - t[old]["us"], 1), added_percent=round(100.0 * (t[new]["us"] / t[old]["us"] - 1.0), 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


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
               front_end=front_rows(lib.kernels, args.rounds, args.iters, args.warmup),
               back_end=back_rows(lib.kernels, args.rounds, args.iters, args.warmup),
               net=net_rows(lib, args.rounds, args.iters, args.warmup))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
