"""Timing of the decode stage in front of the frame path (rt_decode_frames_u8, rt_net_execute_frames_camera).

  1. One pair at 1280x720, every wire encoding into bgr8 and bgra8, dense rows (every base and step a multiple of 4: the dword forms).
     Beside each, timed in the same run: a device-to-device copy of exactly the bytes the launch writes, and rt_rectify_frames_u8 at the
     same size and encoding.  One more row at 1242x375 (rows of 1242 and 3726 bytes: the byte forms) shows what a width off 4 costs.
  2. ResNet-18 2D 1257x369 fp32 (synthetic weights: same kernels as the trained ones) in graph mode on a stream, one 1280x720 pair:
     rt_net_execute_frames_camera from bayer_rggb8 beside rt_net_execute_frames_filtered on already decoded bgr8 frames, disparity out.
  3. With the trained weights, where they are staged: the reference's sample pair as mono8, bayer_rggb8 and yuv422 made by numpy, and the
     mean absolute difference of each disparity from that of the original bgr8 pair (a record, not a bound).

Device events around `iters` (>= 200) launches after warm-up, the compared calls alternated inside one process, `rounds` (>= 5) repeats:
min / median / max of the repeats are recorded with every figure.  Buffers rotate over more than the 256 MB Infinity Cache.
The op's launches take less device time than one call through ctypes takes host time, so a loop of calls measures the host.  The op rows
are therefore timed as a captured graph of the `iters` launches (a chain on one stream, the rotation inside it), replayed between the
events; the same loop issued call by call is recorded beside it as `call_by_call`.

    python tools/time_decode.py [--out profiles/decode.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from redtail_amd import capi, model_files, synth  # noqa: E402
from tools.time_frames_any_size import alternate, rotor  # noqa: E402
from tools.time_rectify import rig  # noqa: E402

H, W = 369, 1257
WIRES = dict(mono8=capi.RT_WIRE_MONO8, mono16=capi.RT_WIRE_MONO16, bayer_rggb8=capi.RT_WIRE_BAYER_RGGB8, bayer_bggr8=capi.RT_WIRE_BAYER_BGGR8,
             bayer_gbrg8=capi.RT_WIRE_BAYER_GBRG8, bayer_grbg8=capi.RT_WIRE_BAYER_GRBG8, yuv422=capi.RT_WIRE_YUV422, yuv422_yuy2=capi.RT_WIRE_YUV422_YUY2)
ENCS = dict(bgr8=capi.RT_ENC_BGR8, bgra8=capi.RT_ENC_BGRA8)


def replayed(k, calls, rounds, iters, sets):
    """{name: dict(us, min_us, max_us)} per launch: each call(i, stream) captured `iters` times with i in rotation into a graph of its own,
    the graphs replayed in turns between device events, `rounds` times after one warm-up replay"""
    s = torch.cuda.Stream()
    st = s.cuda_stream
    graphs, times = {}, {name: [] for name in calls}
    with torch.cuda.stream(s):
        for name, call in calls.items():
            for i in range(sets):
                call(i, st)
            s.synchronize()
            k.check(k.lib.rt_graph_begin_capture(st), "rt_graph_begin_capture")
            for j in range(iters):
                call(j % sets, st)
            graph = ctypes.c_void_p()
            k.check(k.lib.rt_graph_end_capture(st, ctypes.byref(graph)), "rt_graph_end_capture")
            graphs[name] = graph
            k.check(k.lib.rt_graph_launch(graph, st), "rt_graph_launch")
        s.synchronize()
        for _ in range(rounds):
            for name, graph in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                k.check(k.lib.rt_graph_launch(graph, st), "rt_graph_launch")
                b.record(s)
                b.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3 / iters)
    for graph in graphs.values():
        k.lib.rt_graph_destroy(graph)
    return {name: dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for name, v in times.items()}


def op_rows(k, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(6)
    rows = []
    for (h, w), wires in (((720, 1280), WIRES), ((375, 1242), dict(bayer_rggb8=capi.RT_WIRE_BAYER_RGGB8))):
        sets = max(8, int(320e6 / (2 * h * w * 4)) + 1)                  # the rotation of the smallest case (1 byte in, 3 out) > 256 MB
        src = {b: [torch.randint(0, 256, (2, 1, h, w * b), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)] for b in (1, 2)}
        dst = {b: [torch.empty(2, 1, h, w * b, dtype=torch.uint8, device="cuda") for _ in range(sets)] for b in (3, 4)}
        cl, cr = rig(k, h, w, 700.0)
        fns = {}
        for ename, enc in ENCS.items():
            b = capi.ENC_BYTES[enc]
            for wname, wire in wires.items():
                wb = capi.WIRE_BYTES[wire]
                fns["decode_%s_%s" % (wname, ename)] = lambda i, st, a=(src[wb], dst[b], wb, wire, b, enc): k.decode_frames_u8(
                    a[0][i][0], a[0][i][1], h, w, w * a[2], a[3], a[1][i][0], a[1][i][1], w * a[4], a[5], 1, stream=st)
            fns["copy_" + ename] = lambda i, st, a=(dst[b], 2 * h * w * b): k.check(
                k.lib.rt_memcpy_d2d(a[0][i].data_ptr(), a[0][(i + sets // 2) % sets].data_ptr(), a[1], st), "rt_memcpy_d2d")
            fns["rectify_" + ename] = lambda i, st, a=(dst[b], b, enc): k.rectify_frames_u8(
                a[0][(i + sets // 2) % sets][0], a[0][(i + sets // 2) % sets][1], h, w, w * a[1], a[2], cl, cr, a[0][i][0], a[0][i][1], h, w, w * a[1], 1,
                stream=st)
        t = replayed(k, fns, rounds, iters, sets)
        loop = alternate({name: rotor(lambda i, fn=fn: fn(i, None), sets) for name, fn in fns.items()}, rounds, iters, warmup)
        for ename, enc in ENCS.items():
            b = capi.ENC_BYTES[enc]
            copy, rect = t["copy_" + ename], t["rectify_" + ename]
            for wname, wire in wires.items():
                cur, wb = t["decode_%s_%s" % (wname, ename)], capi.WIRE_BYTES[wire]
                row = dict(name="rt_decode_frames_u8 %s -> %s %dx%d, one pair, dense rows" % (wname, ename, w, h), launches=1,
                           form="dword" if w % 4 == 0 else "byte", bytes_read=2 * h * w * wb, bytes_written=2 * h * w * b, sets=sets, **cur,
                           call_by_call=dict(decode=loop["decode_%s_%s" % (wname, ename)], copy=loop["copy_" + ename], rectify=loop["rectify_" + ename]),
                           copy_of_bytes_written=copy, over_copy=round(cur["us"] / copy["us"], 2),
                           gbytes_per_s_moved=round(2 * h * w * (wb + b) / cur["us"] / 1e3, 1), rectify_frames_u8=rect,
                           rectify_over_copy=round(rect["us"] / copy["us"], 2))
                rows.append(row)
                print(json.dumps(row), flush=True)
        del src, dst, fns
        torch.cuda.empty_cache()
    return rows


def net_rows(lib, rounds, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(7)
    s = torch.cuda.Stream()
    k = lib.kernels
    fh, fw = 720, 1280
    net = lib.create("resnet18_2D", W, H, max_batch=1, weights=synth.synth_weights_resnet18_2d())
    net.set_graph(True)
    sets = 8
    wire = [torch.randint(0, 256, (2, 1, fh, fw), dtype=torch.uint8, device="cuda", generator=g) for _ in range(sets)]
    bgr = [torch.empty(2, 1, fh, fw * 3, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    for i in range(sets):
        k.decode_frames_u8(wire[i][0], wire[i][1], fh, fw, fw, capi.RT_WIRE_BAYER_RGGB8, bgr[i][0], bgr[i][1], fw * 3, capi.RT_ENC_BGR8, 1)
    out = [torch.empty(1, 1, fh, fw, device="cuda") for _ in range(3)]
    st = s.cuda_stream
    fns = dict(
        camera=rotor(lambda i: net.execute_frames_camera(wire[i][0], wire[i][1], capi.RT_WIRE_BAYER_RGGB8, capi.RT_ENC_BGR8, disp=out[i % 3], stream=st,
                                                         no_depth_call=True), sets),
        filtered=rotor(lambda i: net.execute_frames_filtered(bgr[i][0], bgr[i][1], capi.RT_ENC_BGR8, disp=out[i % 3], stream=st, src_w=fw,
                                                             no_depth_call=True), sets),
        decode=rotor(lambda i: k.decode_frames_u8(wire[i][0], wire[i][1], fh, fw, fw, capi.RT_WIRE_BAYER_RGGB8, bgr[i][0], bgr[i][1], fw * 3,
                                                  capi.RT_ENC_BGR8, 1, stream=st), sets))
    with torch.cuda.stream(s):                  # events on the same stream as the work
        t = alternate(fns, rounds, iters, warmup)
    torch.cuda.synchronize()
    net.destroy()
    row = dict(model="resnet18_2D", size="%dx%d" % (W, H), engine="fp32", mode="stream+graph", src="%dx%d bayer_rggb8 -> bgr8" % (fw, fh), pairs=1,
               outputs="disparity fp32 at the frame's size", execute_frames_camera=t["camera"], execute_frames_filtered=t["filtered"],
               decode_alone_same_buffers=t["decode"], added_us=round(t["camera"]["us"] - t["filtered"]["us"], 1),
               added_percent=round(100.0 * (t["camera"]["us"] / t["filtered"]["us"] - 1.0), 2))
    print(json.dumps(row), flush=True)
    return [row]


def sample_pair_rows(lib):
    """what decoding costs the trained network on the reference's sample pair: mean |disparity - disparity of the bgr8 pair| in pixels"""
    from PIL import Image
    try:
        weights = model_files.weight_file("resnet18_2D")
        bgr = [np.ascontiguousarray(np.array(Image.open(model_files.sample_image(side)).convert("RGB"))[None, :, :, ::-1]) for side in ("left", "right")]
    except Exception as e:                      # noqa: BLE001  (no staged weights: the timing above stands on its own)
        return dict(skipped=str(e))
    net = lib.create("resnet18_2D", W, H, max_batch=1, weights_path=weights)
    sh, sw = bgr[0].shape[1:3]
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(1, sh, -1)).cuda()

    def disparity(fl, fr, wire):
        out = torch.full((1, 1, sh, sw), float("nan"), device="cuda")
        net.execute_frames_camera(fl, fr, wire, capi.RT_ENC_BGR8, disp=out, no_depth_call=True, src_w=sw)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def uyvy(rgb):
        r, gg, b = (rgb[..., c].astype(np.float64) for c in range(3))
        y = 16 + 0.257 * r + 0.504 * gg + 0.098 * b
        u = (128 - 0.148 * r - 0.291 * gg + 0.439 * b).reshape(1, sh, -1, 2).mean(axis=3)
        v = (128 + 0.439 * r - 0.368 * gg - 0.071 * b).reshape(1, sh, -1, 2).mean(axis=3)
        return np.clip(np.rint(np.stack([u, y[:, :, 0::2], v, y[:, :, 1::2]], axis=3)), 0, 255).astype(np.uint8)

    yy, xx = np.indices((sh, sw))
    channel = np.array([0, 1, 1, 2])[2 * (yy & 1) + (xx & 1)]               # rggb: which of R, G, B a site records
    rgb = [f[..., ::-1] for f in bgr]
    cases = dict(mono8=(capi.RT_WIRE_MONO8, [np.rint(0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]).astype(np.uint8) for f in rgb]),
                 bayer_rggb8=(capi.RT_WIRE_BAYER_RGGB8, [np.take_along_axis(f, channel[None, :, :, None], axis=3) for f in rgb]),
                 yuv422=(capi.RT_WIRE_YUV422, [uyvy(f) for f in rgb]))
    original = disparity(put(bgr[0]), put(bgr[1]), None)
    res = dict(model="resnet18_2D %dx%d fp32, trained weights" % (W, H), pair="the reference's sample pair, %dx%d" % (sw, sh),
               note="mean |disparity - disparity of the bgr8 pair| in frame pixels; wire frames made from the bgr8 pair by numpy")
    for name, (wire, frames) in cases.items():
        res[name] = round(float(np.abs(disparity(put(frames[0]), put(frames[1]), wire) - original).mean()), 4)
    net.destroy()
    print(json.dumps(res), flush=True)
    return res


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
               op=op_rows(lib.kernels, args.rounds, args.iters, args.warmup), net=net_rows(lib, args.rounds, args.iters, args.warmup),
               sample_pair=sample_pair_rows(lib))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
