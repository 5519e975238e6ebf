"""Timing of the first and the last layer of ResNet-18 2D at the timed geometry (1257x369, batch 1), one build beside another.

  conv1 of both towers    conv_s3_first_kernel<true>            2 x (3, 369, 1257) fp32 -> (2, 8, 185, 640, 4)      11.1 MB in, 30.3 MB out
  deconv2D_3              deconv3d_s2_small_kernel<1, false>    (32, 185, 640) fp32 -> (1, 369, 1257), sigmoid      15.2 MB in,  1.9 MB out

The plans are built through the C ABI exactly as tests/test_timed_shapes.py::test_c2_first_layer_twin_input and
::test_c2_last_transposed_layer build them, throughput hint included.  Two settings each: inputs FIXED (cache-hot: how bench.py runs them,
and how deconv2D_3 always finds its input, written by the launch before it) and inputs ROTATING over more than the 256 MB Infinity Cache
(what a camera feeds the first layer).  Device events around `iters` (>= 200) launches after `warmup`, `rounds` (>= 5) windows per
process, the four measurements taking turns: median (min - max) of the windows.

With --against DIR (another build of the two libraries, e.g. the parent commit's; selected with RT_LIB_DIR) the measurement runs in fresh
child processes, that build and this tree's taking turns `reps` times, and every row carries both builds; each child also stores its
outputs for one seeded input per kernel, and the rows record whether the two builds' outputs are equal byte for byte.

    python tools/time_edge_layers.py [--against DIR] [--out profiles/edge_layers.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG_H, IMG_W, H, W, P = 369, 1257, 185, 629, 640
HBM = 8e12                   # bytes / s
ROWS = {
    "first": dict(kernel="conv_s3_first_kernel<true>", layer="conv1 of both towers, twin input", bytes_in=2 * 3 * IMG_H * IMG_W * 4,
                  bytes_out=2 * 32 * H * W * 4),
    "last": dict(kernel="deconv3d_s2_small_kernel<1,false,f32,f32>", layer="deconv2D_3, 32 -> 1, sigmoid", bytes_in=32 * H * W * 4,
                 bytes_out=IMG_H * IMG_W * 4),
}


def child(args):
    import torch
    from redtail_amd import capi
    from tools.time_camera_frames import event_time
    from tools.time_frames_any_size import rotor
    k = capi.KernelLib()
    hint = capi.RT_HINT_THROUGHPUT
    g = torch.Generator(device="cuda").manual_seed(7)
    rn = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float32)
    # -- first layer (test_c2_first_layer_twin_input) --
    w1, b1 = rn(32, 3, 5, 5) / np.sqrt(75), rn(32)
    first = k.conv2d_plan(w1.cpu().numpy(), b1.cpu().numpy(), 3, 32, IMG_H, IMG_W, 5, 2, 2, act=capi.RT_ACT_ELU)
    first.set_pitch(0, P)
    first.set_layouts(0, 1)
    sets1 = int(280e6 / (2 * 3 * IMG_H * IMG_W * 4)) + 1
    imgs = [torch.rand((2, 1, 3, IMG_H, IMG_W), generator=g, device="cuda") for _ in range(sets1)]
    out1 = torch.full((2, 8, H, P, 4), float("nan"), device="cuda")
    # -- last layer (test_c2_last_transposed_layer) --
    wt, bt = rn(32, 1, 3, 3) / np.sqrt(32 * 9 / 4), rn(1)
    last = k.conv2d_plan(wt.cpu().numpy(), bt.cpu().numpy(), 32, 1, H, W, 3, 2, 1, act=capi.RT_ACT_SIGMOID, transposed=True)
    last.set_pitch(P, 0)
    sets2 = int(280e6 / (32 * H * P * 4)) + 1
    maps = [rn(1, 32, H, P) / 10 for _ in range(sets2)]
    out2 = torch.full((1, 1, IMG_H, IMG_W), float("nan"), device="cuda")
    fns = {
        "first/fixed": lambda: first.enqueue_twin_input(imgs[0][0], imgs[0][1], out1, 1, hints=hint),
        "first/rotating": rotor(lambda i: first.enqueue_twin_input(imgs[i][0], imgs[i][1], out1, 1, hints=hint), sets1),
        "last/fixed": lambda: last.enqueue(maps[0], out2, None, 1, hints=hint),
        "last/rotating": rotor(lambda i: last.enqueue(maps[i], out2, None, 1, hints=hint), sets2),
    }
    times = {n: [] for n in fns}
    for _ in range(args.rounds):
        for n, fn in fns.items():
            times[n].append(round(event_time(fn, args.iters, args.warmup) * 1e6, 3))
    # outputs of the seeded inputs of set 0, for the comparison of two builds
    fns["first/fixed"]()
    fns["last/fixed"]()
    torch.cuda.synchronize()
    if args.dump:
        np.savez(args.dump, first=out1.cpu().numpy(), last=out2.cpu().numpy())
    first.destroy()
    last.destroy()
    print("CHILD " + json.dumps(dict(backend=k.backend(), lib=os.path.relpath(k.path, ROOT), times=times, sets=dict(first=sets1, last=sets2))), flush=True)


def run_child(args, lib_dir, dump):
    env = dict(os.environ)
    if lib_dir:
        env["RT_LIB_DIR"] = os.path.abspath(lib_dir)
    else:
        env.pop("RT_LIB_DIR", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds), "--iters", str(args.iters), "--warmup", str(args.warmup),
           "--dump", dump]
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=300)
    if res.returncode != 0:
        raise SystemExit("measurement process failed (%d) with RT_LIB_DIR=%s" % (res.returncode, lib_dir))
    line = [l for l in res.stdout.splitlines() if l.startswith("CHILD ")][-1]
    return json.loads(line[6:])


def summary(v):
    return dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2), windows=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2, help="child processes per build, the builds taking turns")
    ap.add_argument("--against", default="", help="directory of another build of the two libraries (the yardstick)")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--dump", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    builds = ([("against", args.against)] if args.against else []) + [("this", "")]
    times = {b: {} for b, _ in builds}
    info, dumps = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(args.reps):
            for b, d in builds:            # one failed process ends the run: nothing more is started on the device
                dumps[b] = os.path.join(tmp, "%s_%d.npz" % (b, rep))
                r = run_child(args, d, dumps[b])
                info[b] = dict(backend=r["backend"], lib=r["lib"], sets=r["sets"])
                for n, v in r["times"].items():
                    times[b].setdefault(n, []).extend(v)
        equal = None
        if args.against:
            with np.load(dumps["against"]) as a, np.load(dumps["this"]) as t:
                equal = {n: bool(a[n].tobytes() == t[n].tobytes()) for n in ("first", "last")}
    rows = []
    for name in ("first/fixed", "first/rotating", "last/fixed", "last/rotating"):
        key, setting = name.split("/")
        meta = ROWS[key]
        nbytes = meta["bytes_in"] + meta["bytes_out"]
        row = dict(name=name, inputs=setting, **meta, bytes_moved=nbytes, us_at_8TBps=round(nbytes / HBM * 1e6, 2))
        for b, _ in builds:
            s = summary(times[b][name])
            s["fraction_of_8TBps"] = round(nbytes / (s["us"] * 1e-6) / HBM, 3)
            row[b] = s
        if args.against:
            a, t = row["against"], row["this"]
            row["outputs_byte_equal"] = equal[key]
            row["below_yardstick_min"] = bool(t["us"] < a["min_us"])
            row["lower_by_more_than_yardstick_spread"] = bool(a["us"] - t["us"] > a["max_us"] - a["min_us"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(rounds=args.rounds, iters=args.iters, warmup=args.warmup, reps=args.reps, builds=info,
               note="us = median of the windows of `iters` launches between device events (`rounds` per process, `reps` processes per build, the "
                    "builds taking turns); min_us / max_us = their spread; 'against' = the yardstick build, 'this' = this tree's",
               rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
