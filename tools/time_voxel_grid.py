"""Timing of the voxel grid (rt_points_voxel_grid, rt_net_execute_frames_voxels).

  1. The op alone at 1242x375 on a realistic cloud: the reference's sample pair through ResNet-18 2D 1257x369 (trained weights where they
     are staged, synthetic ones otherwise: the JSON says which) with a check at 1 px and rt_disparity_to_points under a KITTI calibration.
     Leaves of 0.1 m (400 x 50 x 800 cells) and 0.05 m (800 x 100 x 1600 = 128 M cells, close to the op's limit), batch 1 and 8 (the same
     cloud in every image), on the organised cloud (count == NULL) and on the compact one.  Beside it, timed in the same run: a
     device-to-device copy of the bytes the op reads, and the device-to-host copy of the full organised cloud into pinned memory -- the
     transfer a host-side pcl::VoxelGrid needs and this op makes unnecessary.
  2. The entry in graph mode on a stream, one 1242x375 bgr8 pair, check on: rt_net_execute_frames_voxels with no cloud output beside
     rt_net_execute_frames_camera with the compact cloud (what a caller of a host-side voxel filter asks for).

Device events around `iters` (>= 200) launches after warm-up, the compared calls alternated inside one process, `rounds` (>= 5) repeats:
min / median / max of the repeats are recorded with every figure.  Buffers rotate over more than the 256 MB Infinity Cache.

    python tools/time_voxel_grid.py [--out profiles/voxel_grid.json]
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
from tools.time_frames_any_size import alternate, rotor  # noqa: E402

H, W, FH, FW = 369, 1257, 375, 1242
KITTI = dict(fx=721.5377, fy=721.5377, cx=609.5593, cy=172.854, baseline=0.54)
GRIDS = {0.1: capi.VoxelGrid.make((-20.0, -2.5, 0.0), 0.1, (400, 50, 800)), 0.05: capi.VoxelGrid.make((-20.0, -2.5, 0.0), 0.05, (800, 100, 1600))}


def sample_frames():
    from PIL import Image
    return [torch.from_numpy(np.ascontiguousarray(np.array(Image.open(model_files.sample_image(side)).convert("RGB"))[None, :, :, ::-1])).cuda()
            for side in ("left", "right")]


def make_net(lib):
    try:
        return lib.create("resnet18_2D", W, H, max_batch=2, weights_path=model_files.weight_file("resnet18_2D")), "trained"
    except FileNotFoundError:
        return lib.create("resnet18_2D", W, H, max_batch=2, weights=synth.synth_weights_resnet18_2d()), "synthetic"


def op_rows(k, cloud, compact, count, rounds, iters, warmup):
    rows = []
    pixels = FH * FW
    for leaf, grid in GRIDS.items():
        for batch in (1, 8):
            ws_bytes = k.voxel_workspace_bytes(batch, pixels, grid)
            sets = max(2, int(320e6 / (ws_bytes + batch * pixels * 40)) + 1)
            org = [cloud.repeat(batch, 1, 1).contiguous() for _ in range(sets)]
            cmp_ = [compact.repeat(batch, 1, 1).contiguous() for _ in range(sets)]
            cnt = count.repeat(batch).contiguous()
            ws = [torch.empty(ws_bytes, dtype=torch.uint8, device="cuda") for _ in range(sets)]
            vox = [torch.empty(batch, pixels, 16, dtype=torch.uint8, device="cuda") for _ in range(sets)]
            ocnt = [torch.zeros(batch, dtype=torch.int64, device="cuda") for _ in range(sets)]
            dst = [torch.empty(batch, pixels, 16, dtype=torch.uint8, device="cuda") for _ in range(sets)]
            host = torch.empty(batch, pixels, 16, dtype=torch.uint8).pin_memory()

            def organised(i, min_points=1):
                k.points_voxel_grid(org[i], batch, pixels, grid, vox[i], pixels, ocnt[i], min_points=min_points, workspace=ws[i])

            def compacted(i):
                k.points_voxel_grid(cmp_[i], batch, pixels, grid, vox[i], pixels, ocnt[i], count=cnt, workspace=ws[i])

            def copy(i):
                k.check(k.lib.rt_memcpy_d2d(dst[i].data_ptr(), org[i].data_ptr(), batch * pixels * 16, None), "rt_memcpy_d2d")

            def d2h(i):
                host.copy_(org[i], non_blocking=True)

            organised(0)
            torch.cuda.synchronize()
            voxels = int(ocnt[0][0].item())
            fns = dict(organised=rotor(organised, sets), compact=rotor(compacted, sets), min_points_3=rotor(lambda i: organised(i, 3), sets),
                       copy=rotor(copy, sets), d2h=rotor(d2h, sets))
            t = alternate(fns, rounds, iters, warmup)
            row = dict(name="rt_points_voxel_grid %dx%d batch %d, leaf %g m, %d x %d x %d cells" % ((FW, FH, batch, leaf) + tuple(grid.dims)),
                       batch=batch, leaf_m=leaf, cells=int(np.prod(list(grid.dims))), sets=sets, launches=6, launches_min_points_3=8,
                       records_per_image=pixels, valid_points_per_image=int(count.item()), voxels_per_image=voxels,
                       bytes_read=batch * pixels * 16, workspace_bytes=int(ws_bytes), organised=t["organised"], compact=t["compact"],
                       organised_min_points_3=t["min_points_3"], copy_of_bytes_read=t["copy"], d2h_of_the_organised_cloud=t["d2h"],
                       over_copy=round(t["organised"]["us"] / t["copy"]["us"], 2), over_d2h=round(t["organised"]["us"] / t["d2h"]["us"], 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del org, cmp_, ws, vox, ocnt, dst, host
            torch.cuda.empty_cache()
    return rows


def net_rows(net, frames, cam, rounds, iters, warmup):
    s = torch.cuda.Stream()
    g = torch.Generator(device="cuda").manual_seed(5)
    net.set_graph(True)
    sets, pixels = 8, FH * FW
    base = torch.stack([f.reshape(1, FH, FW * 3) for f in frames])
    ring = []
    for i in range(sets):                                  # the same scene with a little noise: other bytes behind other pointers
        noise = torch.randint(0, 3, base.shape, dtype=torch.uint8, device="cuda", generator=g)
        ring.append(torch.clamp(base.to(torch.int16) + noise.to(torch.int16) - 1, 0, 255).to(torch.uint8))
    cloud = [torch.empty(1, pixels, 16, dtype=torch.uint8, device="cuda") for _ in range(3)]
    count = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(3)]
    vox = [torch.empty(1, pixels, 16, dtype=torch.uint8, device="cuda") for _ in range(3)]
    vcount = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(3)]
    st = s.cuda_stream
    grid = GRIDS[0.05]

    def camera(i):
        net.execute_frames_camera(ring[i][0], ring[i][1], None, capi.RT_ENC_BGR8, camera=cam, max_diff_px=1.0, min_depth=0.5, max_depth=80.0,
                                  points_compact=cloud[i % 3], count=count[i % 3], stream=st, src_w=FW)

    def voxels(i):
        net.execute_frames_voxels(ring[i][0], ring[i][1], capi.RT_ENC_BGR8, grid=grid, voxels=vox[i % 3], voxel_count=vcount[i % 3], camera=cam,
                                  max_diff_px=1.0, min_depth=0.5, max_depth=80.0, stream=st, src_w=FW)

    fns = dict(voxels=rotor(voxels, sets), camera=rotor(camera, sets))
    with torch.cuda.stream(s):                  # events on the same stream as the work
        camera(0)
        voxels(0)
        s.synchronize()
        points, emitted = int(count[0].item()), int(vcount[0].item())
        t = alternate(fns, rounds, iters, warmup)
    torch.cuda.synchronize()
    row = dict(model="resnet18_2D", size="%dx%d" % (W, H), engine="fp32", mode="stream+graph", src="1242x375 bgr8", pairs=1, check="1 px",
               leaf_m=0.05, cells=int(np.prod(list(grid.dims))), voxels_entry=t["voxels"], camera_entry_compact_cloud=t["camera"],
               added_us=round(t["voxels"]["us"] - t["camera"]["us"], 1), added_percent=round(100.0 * (t["voxels"]["us"] / t["camera"]["us"] - 1.0), 2),
               cloud_points=points, voxels=emitted, cloud_bytes=points * 16, voxel_bytes=emitted * 16)
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
    net, weights = make_net(lib)
    frames = sample_frames()
    cam = capi.StereoCamera(KITTI["fx"], KITTI["fy"], KITTI["cx"], KITTI["cy"], KITTI["baseline"], 0.0)
    pixels = FH * FW
    cloud = torch.empty(1, pixels, 16, dtype=torch.uint8, device="cuda")
    compact = torch.zeros(1, pixels, 16, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    net.execute_frames_camera(frames[0].reshape(1, FH, FW * 3), frames[1].reshape(1, FH, FW * 3), None, capi.RT_ENC_BGR8, camera=cam, max_diff_px=1.0,
                              min_depth=0.5, max_depth=80.0, points=cloud, points_compact=compact, count=count, src_w=FW)
    torch.cuda.synchronize()
    res = dict(backend=lib.kernels.backend(), rounds=args.rounds, iters=args.iters, warmup=args.warmup, weights=weights,
               note="us = median of `rounds` windows of `iters` launches between device events; min_us / max_us = their spread",
               op=op_rows(lib.kernels, cloud, compact, count, args.rounds, args.iters, args.warmup),
               net=net_rows(net, frames, cam, args.rounds, args.iters, args.warmup))
    net.destroy()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
