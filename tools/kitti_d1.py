#!/usr/bin/env python3
"""D1 error of a Stereo DNN model on the KITTI 2015 stereo training set (200 pairs), end to end on the GPU:
PNG -> one rt_net_execute_frames_ex per pair (RT_RESIZE_CV_AREA: cv::resize(INTER_AREA) to the network size, growing axes included;
RT_GEOM_FRAME: disparity in the pixels and the geometry of the original image).

    python tools/kitti_d1.py <kitti>/training  <trt_weights.bin>  [--model resnet18_2D] [--width 1257 --height 369]

The default size is the headline configuration for resnet18_2D and the size the reference ships for the other models.

The reference quotes 9.8 % (ResNet-18 2D), 7.7 % (NVSmall), 11.1 % (NVTiny) in stereoDNN/README.md:26-36.
Needs the dataset (not redistributable) and an MI355X; nothing of this runs in the test suites."""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from redtail_amd import capi, kitti  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("root")
    ap.add_argument("weights")
    ap.add_argument("--model", default="resnet18_2D")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    args = ap.parse_args()
    default = {"resnet18_2D": (1257, 369), "nvtiny": (513, 161)}.get(args.model, (1025, 321))
    args.width, args.height = args.width or default[0], args.height or default[1]
    lib = capi.NetLib()
    net = lib.create(args.model, args.width, args.height, weights_path=args.weights)
    lefts = sorted(glob.glob(os.path.join(args.root, "image_2", "*_10.png")))
    if not lefts:
        sys.exit("no image_2/*_10.png under %s" % args.root)
    scores = []
    for lp in lefts:
        name = os.path.basename(lp)
        l8 = torch.from_numpy(kitti.read_image_bgr(lp)).cuda()[None]
        r8 = torch.from_numpy(kitti.read_image_bgr(os.path.join(args.root, "image_3", name))).cuda()[None]
        h, w = l8.shape[1:3]
        d = torch.empty(1, 1, h, w, device="cuda")          # KITTI frames differ in size by a few pixels: one output per pair
        net.execute_frames_ex(l8, r8, capi.RT_ENC_BGR8, d, kind=capi.RT_DISP_PIXELS_F32, geometry=capi.RT_GEOM_FRAME,
                              resize=capi.RT_RESIZE_CV_AREA)
        d = d[0, 0]
        gt = kitti.read_disparity_png(os.path.join(args.root, "disp_occ_0", name))
        scores.append(kitti.d1_all(d.cpu().numpy(), gt))
        print("%s  D1 %.2f %%" % (name, scores[-1]), flush=True)
    print("mean D1-all over %d pairs: %.2f %%" % (len(scores), float(np.nanmean(scores))))


if __name__ == "__main__":
    main()
