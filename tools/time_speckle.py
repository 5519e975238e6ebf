"""Timing of the speckle filter (rt_disparity_speckle, rt_net_execute_frames_filtered).

  1. 1257x369, batch 1 and 8, on a synthetic checked disparity with a realistic hole pattern (synth.synth_speckle_disparity: out-of-view
     band, occlusion bands, pinholes, small islands inside the holes), speckle_size 200 / speckle_range 1: rt_disparity_speckle.
     Beside it, timed in the same run: rt_lr_consistency on an engine output of the same size and batch, a device-to-device copy of the bytes the filter reads and writes (5 per pixel each way), and the filter with max_size 0 (its last
     launch alone).
  2. ResNet-18 2D 1257x369 fp32 (synthetic weights: same kernels as the trained ones) in graph mode on a stream, one 1242x375 bgr8 pair,
     check on, disparity + depth + compact cloud: rt_net_execute_frames_filtered with a filter beside the same call without one.

Device events around `iters` (>= 200) launches after warm-up, the compared calls alternated inside one process, `rounds` (>= 5) repeats:
min / median / max of the repeats are recorded with every figure.  Buffers rotate over more than the 256 MB Infinity Cache.

    python tools/time_speckle.py [--out profiles/speckle.json]
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
MAX_SIZE, MAX_DIFF = 200, 1.0


def op_rows(k, rounds, iters, warmup):
    rows = []
    for batch in (1, 8):
        px, mask = synth.synth_speckle_disparity(batch, H, W)
        pixels = batch * H * W
        sets = max(8, int(320e6 / (pixels * 18)) + 1)      # per set: disparity, mask, workspace (8 per pixel) and the copy's target
        src_px, src_mask = torch.from_numpy(px).cuda(), torch.from_numpy(mask).cuda()
        pxs = [src_px.clone() for _ in range(sets)]
        masks = [src_mask.clone() for _ in range(sets)]
        ws = [torch.empty(k.speckle_workspace_bytes(batch, H, W), dtype=torch.uint8, device="cuda") for _ in range(sets)]
        dst = [torch.empty(pixels * 5, dtype=torch.uint8, device="cuda") for _ in range(sets)]
        net_disp = [torch.rand(2 * batch, 1, H, W, device="cuda") * 0.05 for _ in range(sets)]
        lr_out = [torch.empty(batch, 1, H, W, device="cuda") for _ in range(sets)]
        lr_mask = [torch.empty(batch, 1, H, W, dtype=torch.uint8, device="cuda") for _ in range(sets)]

        def copy(i):
            k.check(k.lib.rt_memcpy_d2d(dst[i].data_ptr(), pxs[i].data_ptr(), pixels * 4, None), "rt_memcpy_d2d")
            k.check(k.lib.rt_memcpy_d2d(dst[i].data_ptr() + pixels * 4, masks[i].data_ptr(), pixels, None), "rt_memcpy_d2d")

        def lr(i):
            k.lr_consistency(net_disp[i], batch, H, W, float(W), 1.0, lr_out[i], capi.RT_DISP_PIXELS_F32, lr_mask[i], None, None)

        # out of place, so that every timed call meets the unfiltered image (in place, the second call would find no speckle left): the
        # same launches and the same bytes as the frame path's in-place call, the output elsewhere
        outs = [torch.empty(batch, 1, H, W, device="cuda") for _ in range(sets)]
        omasks = [torch.empty(batch, 1, H, W, dtype=torch.uint8, device="cuda") for _ in range(sets)]

        def speckle_fresh(i, max_size=MAX_SIZE):
            k.disparity_speckle(pxs[i], batch, H, W, max_size, MAX_DIFF, outs[i], mask=masks[i], out_mask=omasks[i], workspace=ws[i])

        speckle_fresh(0)
        torch.cuda.synchronize()
        kept = int((omasks[0] != 0).sum())
        fns = dict(speckle=rotor(speckle_fresh, sets), speckle_max_size_0=rotor(lambda i: speckle_fresh(i, 0), sets), lr_consistency=rotor(lr, sets), copy=rotor(copy, sets))
        t = alternate(fns, rounds, iters, warmup)
        live = int((mask != 0).sum())
        row = dict(name="rt_disparity_speckle %dx%d batch %d, max_size %d, max_diff_px %g" % (W, H, batch, MAX_SIZE, MAX_DIFF), batch=batch,
                   launches=4, sets=sets, live_pixels=live, removed_pixels=live - kept, bytes_read=pixels * 5, bytes_written=pixels * 5,
                   workspace_bytes=int(ws[0].numel()), **t["speckle"],
                   max_size_0_one_launch=t["speckle_max_size_0"], lr_consistency_same_size=t["lr_consistency"], copy_of_bytes_read_and_written=t["copy"],
                   over_lr_consistency=round(t["speckle"]["us"] / t["lr_consistency"]["us"], 2), over_copy=round(t["speckle"]["us"] / t["copy"]["us"], 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pxs, masks, ws, dst, net_disp, lr_out, lr_mask, outs, omasks
        torch.cuda.empty_cache()
    return rows


def net_rows(lib, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(5)
    s = torch.cuda.Stream()
    net = lib.create("resnet18_2D", W, H, max_batch=2, weights=synth.synth_weights_resnet18_2d())
    net.set_graph(True)
    sets = 8
    cam = capi.StereoCamera(721.5, 721.5, (FW - 1) / 2 + 1.7, (FH - 1) / 2 - 0.9, 0.54, 0.0)
    left, right = (np.clip(img.transpose(1, 2, 0)[:, :, ::-1] * 255.0 + 0.5, 0, 255).astype(np.uint8) for img in synth.synth_pair(FH, FW))
    base = torch.from_numpy(np.stack([left.reshape(FH, FW * 3), right.reshape(FH, FW * 3)])[:, None]).cuda()
    frames = []
    for i in range(sets):                                  # the same scene with a little noise: other bytes behind other pointers
        noise = torch.randint(0, 3, base.shape, dtype=torch.uint8, device="cuda", generator=g)
        frames.append(torch.clamp(base.to(torch.int16) + noise.to(torch.int16) - 1, 0, 255).to(torch.uint8))
    out_f = [torch.empty(1, 1, FH, FW, device="cuda") for _ in range(3)]
    depth = [torch.empty(1, 1, FH, FW, device="cuda") for _ in range(3)]
    cloud = [torch.empty(1, FH, FW, 4, device="cuda") for _ in range(3)]
    count = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(3)]
    vcount = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(3)]
    st = s.cuda_stream

    def call(i, size):
        net.execute_frames_filtered(frames[i][0], frames[i][1], capi.RT_ENC_BGR8, speckle_size=size, speckle_range=MAX_DIFF, camera=cam,
                                    disp=out_f[i % 3], max_diff_px=1.0, valid_count=vcount[i % 3], min_depth=0.5, max_depth=80.0, depth=depth[i % 3],
                                    points_compact=cloud[i % 3], count=count[i % 3], stream=st, src_w=FW)

    fns = dict(filtered=rotor(lambda i: call(i, MAX_SIZE), sets), unfiltered=rotor(lambda i: call(i, None), sets))
    with torch.cuda.stream(s):                  # events on the same stream as the work
        call(0, None)
        s.synchronize()
        valid_plain, points_plain = int(vcount[0].item()), int(count[0].item())
        call(0, MAX_SIZE)
        s.synchronize()
        valid_filtered, points_filtered = int(vcount[0].item()), int(count[0].item())
        t = alternate(fns, rounds, iters, warmup)
    torch.cuda.synchronize()
    net.destroy()
    row = dict(model="resnet18_2D", size="%dx%d" % (W, H), engine="fp32", mode="stream+graph", src="1242x375 bgr8", pairs=1, check="1 px",
               outputs="disparity fp32 + depth fp32 + compact cloud", max_size=MAX_SIZE, max_diff_px=MAX_DIFF, filtered=t["filtered"],
               unfiltered=t["unfiltered"], added_us=round(t["filtered"]["us"] - t["unfiltered"]["us"], 1),
               added_percent=round(100.0 * (t["filtered"]["us"] / t["unfiltered"]["us"] - 1.0), 2),
               valid_pixels=dict(unfiltered=valid_plain, filtered=valid_filtered), cloud_points=dict(unfiltered=points_plain, filtered=points_filtered))
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
