#!/usr/bin/env python3
"""Headline benchmark: stereo pairs/sec of ResNet-18 2D Stereo DNN, fp32, 1257x369, batch 1 per step.

    python bench.py --gpus N --steps K --warmup W [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps, writes --dump-outputs if asked and prints the JSON line: the headline
figure and what describes its set-up, nothing else.  --full adds everything else this file measures or checks, after the
timed region as before: `single_context`, the objects listed below, the oracle parity of what was timed (`parity_max_abs_err`), the bitwise
agreement of the contexts (`contexts_max_abs_diff`) and, on the 3-D lines, the roofline.

One rank per GPU.  A "step" = one IExecutionContext::enqueue of one stereo pair through the whole
network (23 launches at this size) with the inputs already resident in HBM (the reference times
context->execute the same way, sample_app/main.cpp:303-309).  Steps are issued round-robin over
--contexts execution contexts of the same engine configuration, each on its own stream (default 3 with one
HIP stream each, the TensorRT throughput set-up `trtexec --streams`): the serial low-resolution tail of one pair
then overlaps the encoder of the next.  "single_context" on the JSON line is the same workload through one
context with two streams (the latency set-up), "synchronous_execute" the reference's own loop.  Stereo pairs are independent, so ranks
share nothing but the weights: rank 0 builds the weight-file image and broadcasts it over RCCL
(torch.distributed backend "nccl"); there is no data-path collective and scaling is weak (each rank
processes its own K pairs).

Extra objects on the JSON line (--full only):
  roofline      dominant kernel = conv_s3rbd_kernel (round 6; conv_s3rbs_kernel with RT_NO_RBD=1), one launch per residual block of the feature towers over both images (the 32
                3x3 32->32 convolutions at 629x185 = 79 % of the network's FLOPs, ~55-60 % of its GPU time; layer by layer with
                RT_RB=0: conv_s3_kernel<3,3,1,il,il>): fp32 tensors, 3-term fp16 split on
                v_mfma_f32_32x32x16_f16 with fp32 accumulation.  At 16x the fp32 matrix rate the layer is bound by moving its
                tensors, so the object is priced in ALGORITHMIC bytes per launch (x + residual + y + weights + bias, each once,
                SURVEY.md 8d) / average launch duration measured with HIP events on the launch stream (IProfiler path of the
                executor) right after the timed region, against 8 TB/s.  `traffic` = HBM bytes per launch from the committed
                PMC passes (profiles/rNN_traffic.json).  RT_CONV_EXACT_FP32=1 (round 1's fp32 Winograd kernel) is priced in
                direct-form FLOPs against the fp32 matrix peak instead; --half2 (TensorRT half2 mode, BASELINE config C3) in
                fp16 bytes.
                `frac` uses the in-situ duration (event pairs inside the running network, other streams busy);
                `isolated_launch_us` / `frac_isolated` are the same layer launched back-to-back on an idle GPU; `frac_step`
                and `frac_of_fp32_mfma_peak*` put the step and the launch on round 1's scale (direct-form FLOPs / 157.3 TFLOP/s).
  cpu_baseline  the oracle (torch CPU restatement of the reference graph, oracle/stereo_oracle.py) timed
                on this host's cores on a bounded sample of the same workload.
  latency_ms_per_pair   IExecutionContext::execute() in a loop, one context: the reference's own timing protocol (`ms_per_pair` is
                1 / throughput with several pairs in flight)
  value_200 / value_exact_fp32   the same set-up over 200 steps / with RT_CONV_EXACT_FP32=1 (fp32 fmaf-chain kernels, no fp16 split)
  secondary     `--full` with N = 1 and no other flags: BASELINE configs C3, C5, C4, the reference's published 513x257 configuration and
                NVTiny 513x161 (C1), each a bounded run with its own parity check against the oracle on one pair, outside the timed
                region (--no-secondary skips them)
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from redtail_amd import capi, parallel, synth  # noqa: E402

W, H = 1257, 369
MFMA_F32_PEAK_TFLOPS = 157.3          # /opt/skills/guides/MI355X_MICROARCH.md, chip-level parameters
HBM_PEAK_GBS = 8000.0                 # same table: HBM3E, 8 TB/s
MFMA_F16_PEAK_TFLOPS = 2500.0         # same table: dense fp16 / bf16 matrix peak
HALF_W, HALF_H = 629, 185
DOMINANT_FLOPS = 2.0 * 32 * 32 * 9 * HALF_W * HALF_H      # one 3x3 32->32 conv at half resolution
DOMINANT_BYTES = 4.0 * (3 * 32 * HALF_W * HALF_H + 32 * 32 * 9 + 32)     # x, residual, y, weights, bias
NET_FLOPS = 91.87e9                    # whole network per pair at 1257x369, direct form


def net_bytes_2d():
    """ALGORITHMIC HBM bytes of one pair through the 48 launches of ResNet-18 2D at 1257x369, fp32: every launch reads its input
    (+ skip tensor) and writes its output once (weights are noise: 2.9 MB in all)."""
    px = lambda c, h, w: 4.0 * c * h * w
    h2, w2, h4, w4, h8, w8, h16, w16 = HALF_H, HALF_W, 93, 315, 47, 158, 24, 79
    t = px(32, h2, w2)
    total = 2 * (px(3, H, W) + t)                              # conv1, left / right
    total += 32 * 3 * t - 16 * t                               # 32 residual-block convolutions: x, y (+ skip on every second one)
    total += 2 * 2 * t                                         # encoder2D_out x 2
    total += 2 * t + px(1, h2, w2)                             # correlation + soft-argmax
    total += px(33, h2, w2) + t + 2 * t                        # conv2D_1, conv2D_2
    total += t + px(64, h4, w4) + 2 * 2 * px(64, h4, w4)       # conv2D_3ds, conv2D_4, conv2D_5
    total += px(64, h4, w4) + px(128, h8, w8) + 2 * 2 * px(128, h8, w8)      # conv2D_6ds, conv2D_7, conv2D_8
    total += px(128, h8, w8) + 2 * px(64, h4, w4)              # deconv2D_1 (+ skip)
    total += px(64, h4, w4) + 2 * t                            # deconv2D_2 (+ skip)
    total += t + px(1, H, W)                                   # deconv2D_3
    return total



def load_weights(half2):
    """(dict, description) of the timed weights: seeded synthetic, so that the inputs of a run -- and with --dump-outputs its outputs --
    depend on the arguments alone (the reference's trained files are exercised by tests/test_net_parity.py).  In half2 mode the engine
    rounds them to fp16 as it would the reference's fp16 file."""
    return synth.synth_weights_resnet18_2d(seed=7), "seeded He-normal (synthetic)"


def dominant(name):
    return "resblock" in name


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(dirname, arrays):
    """--dump-outputs: writes every array as DIR/<name>.npy in float32.  An array beyond its share of the 64 MB budget is replaced
    by a seeded sample of its elements (flattened, ascending positions): the same positions for the same shape on every run."""
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(1, len(arrays))
    for name, t in arrays.items():
        a = t.detach().cpu().numpy().astype(np.float32)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), a)


# a fused residual block (conv_s3rb_kernel): two of the 3x3 convolutions, x read once (with its halo), y written once
BLOCK_FLOPS = 2.0 * DOMINANT_FLOPS
BLOCK_BYTES = 4.0 * (2 * 32 * HALF_W * HALF_H + 2 * (32 * 32 * 9 + 32))


NATIVE_STARTUP_HUNG = [False]       # main(): the native multi-GPU start-up was abandoned in its thread -> leave with os._exit after the JSON line


def measured_traffic(half2=False, fused=None):
    """HBM bytes per launch of the dominant kernel from the newest committed PMC pass (profiles/rNN_traffic.json,
    written by tools/summarize_profiles.py from separate `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` runs of this
    command; counters cannot be read from inside the timed process).  None when no such file is present."""
    import glob
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")) if ("half2" in os.path.basename(f)) == half2)
    if not files:
        return None, None
    t = json.load(open(files[-1]))
    if fused is not None and ("conv_s3rb" in t.get("kernel", "")) != fused:
        return None, None                                   # the PMC pass was taken with the other kernel as the dominant one
    if t.get("sources_sha16") not in (None, kernel_sources_sha16()):
        return None, "%s is stale: taken on kernel sources %s, these are %s" % (os.path.relpath(files[-1], ROOT), t.get("sources_sha16"), kernel_sources_sha16())
    src = os.path.relpath(files[-1], ROOT)
    if "images_per_launch" in t:            # what a counted launch covers (since round 3: both towers' samples of a block) and its algorithmic bytes
        src += "; counted launches cover %d image(s): %.1f MB algorithmic" % (
            t["images_per_launch"], (t["algorithmic_read_bytes"] + t["algorithmic_write_bytes"]) / 1e6)
    return t["hbm_bytes_per_launch"], src


def kernel_sources_sha16():
    """Hash of the kernel sources the counters of profiles/rNN_traffic.json belong to (tools/summarize_profiles.py stamps the file)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "redtail_amd", "csrc", "kernels", "*.h"))) + [os.path.join(ROOT, "redtail_amd", "csrc", "rt_capi.hip")]:
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def make_streams(klib, n, dev):
    """n NON-BLOCKING HIP streams (rt_stream_create = hipStreamNonBlocking), wrapped for torch.  torch.cuda.Stream() makes blocking
    streams, and every operation on the legacy NULL stream -- IExecutionContext::execute() orders itself after it -- then pays for
    each of them (852 vs 606 us per pair in the synchronous loop with this process's eight streams)."""
    import ctypes
    out = []
    for _ in range(n):
        h = ctypes.c_void_p()
        klib.check(klib.lib.rt_stream_create(ctypes.byref(h)), "rt_stream_create")
        out.append(torch.cuda.ExternalStream(h.value, device=dev))
    return out


def host_cores():
    """Cores this process may really use: the cgroup CPU quota if there is one, else the affinity mask."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(weights, budget_s=12.0):
    """Bounded CPU sample of the same workload through the oracle (kind = "port")."""
    from oracle import stereo_oracle as O
    torch.set_num_threads(host_cores())                     # more threads than the quota only adds throttling
    l, r = synth.synth_pair(H, W, 1234)
    L, R = torch.from_numpy(l)[None], torch.from_numpy(r)[None]
    with torch.no_grad():
        O.resnet18_2d(L, R, weights)                        # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            O.resnet18_2d(L, R, weights)
            n += 1
            dt = time.perf_counter() - t0
            if dt >= budget_s or n >= 512:
                break
    out = dict(value=n / dt, unit="pairs/s", cores=torch.get_num_threads(), kind="port",
               sample="%d pairs of 1257x369 in %.1f s, torch %s CPU fp32 oracle" % (n, dt, torch.__version__))
    # the same oracle on ONE core (what a scalar port would be measured as): a few pairs
    torch.set_num_threads(1)
    with torch.no_grad():
        n1, t1 = 0, time.perf_counter()
        while n1 < 2 or time.perf_counter() - t1 < 4.0:
            O.resnet18_2d(L, R, weights)
            n1 += 1
        d1 = time.perf_counter() - t1
    torch.set_num_threads(host_cores())
    out["one_core"] = dict(value=n1 / d1, unit="pairs/s", cores=1, sample="%d pairs in %.1f s" % (n1, d1))
    return out


def isolated_dominant(k, b, half2, launches=50, fused=False, hints=0):
    """The dominant layer (3x3 32->32 @629x185 + bias + residual + ELU, the executor's tensor layouts) launched
    back-to-back on one idle stream: microseconds per launch between two HIP events.  Reported next to the in-situ
    figure (`avg_launch_us`: event pairs inside the running network, other streams' kernels in flight)."""
    import ctypes
    rng = np.random.default_rng(1)
    wt = (rng.standard_normal((32, 32, 3, 3)) / np.sqrt(288)).astype(np.float32)
    if fused:
        plan = k.resblock_plan(wt, rng.standard_normal(32).astype(np.float32), wt[::-1].copy(), rng.standard_normal(32).astype(np.float32),
                               32, 32, HALF_H, HALF_W)
    else:
        plan = k.conv2d_plan(wt, rng.standard_normal(32).astype(np.float32), 32, 32, HALF_H, HALF_W, 3, 1, 1, act=capi.RT_ACT_ELU, has_residual=True)
    plan.set_pitch(640, 640)
    if half2:
        plan.set_io_types(capi.RT_F16, capi.RT_F16)
    if plan.supports_il8():
        plan.set_layouts(1, 1, 1)
    dt = torch.float16 if half2 else torch.float32
    x = torch.randn(b, 32, HALF_H, 640, device="cuda").to(dt)
    if fused and not half2 and plan.supports_split():
        # the typical tower block reads and writes PRE-SPLIT tensors (rt_resblock_plan_set_split): (C/8, H, pitch, [8 hi | 8 lo]) fp16 pairs
        plan.set_split(1, 1)
        g = x.reshape(b, 4, 8, HALF_H, 640).permute(0, 1, 3, 4, 2)
        hi = g.half()
        x = torch.cat([hi, ((g - hi.float()) * 2048.0).half()], dim=-1).contiguous().view(torch.float32)
    r, y = (x if fused else torch.randn_like(x)), torch.empty_like(x)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    k.lib.rt_event_create(ctypes.byref(e0)); k.lib.rt_event_create(ctypes.byref(e1))
    for _ in range(5):
        plan.enqueue(x, y, r, b, hints=hints)
    torch.cuda.synchronize()
    k.lib.rt_event_record(e0, None)
    for _ in range(launches):
        plan.enqueue(x, y, r, b, hints=hints)
    k.lib.rt_event_record(e1, None)
    torch.cuda.synchronize()
    ms = ctypes.c_float()
    k.lib.rt_event_elapsed_ms(e0, e1, ctypes.byref(ms))
    k.lib.rt_event_destroy(e0); k.lib.rt_event_destroy(e1)
    plan.destroy()
    return ms.value * 1e3 / launches



# ---- the 3-D models (BASELINE configs C4 / C5): `--model nvsmall|resnet18|nvtiny [--half2] [--batch B]` --------------------------
MODELS_3D = {"nvtiny": (513, 161, 24, "NVTINY_3D"), "nvsmall": (1025, 321, 48, "NVSMALL_3D"), "resnet18": (1025, 321, 68, "RESNET18_3D")}


FLOPS_3D = {}          # filled by trunk_bytes_3d: direct-form FLOPs per pair and 3-D layer


def trunk_bytes_3d(cfg, h, w, max_disp, es):
    """ALGORITHMIC HBM bytes of the 3-D trunk per pair: every fused Conv3D / Conv3DTranspose launch reads its input (the first
    one gathers the two 2-D feature maps instead of a cost volume), its skip tensor if it has one, and writes its output, each
    once; `es` = bytes per element of the 4-D tensors (2 in half2 mode), the last layer's volume is fp32.  Returns (total,
    {layer: bytes})."""
    H, W, D = (h + 1) // 2, (w + 1) // 2, max_disp
    dims = {}
    per = {}
    cur = None
    half = lambda n: (n + 1) // 2
    for i, (name, k, c, stride) in enumerate(cfg["conv3d"]):
        if stride == 2:
            D, H, W = half(D), half(H), half(W)
        out = k * D * H * W
        rd = (2 * cfg["feat"] * ((h + 1) // 2) * ((w + 1) // 2) * 4) if i == 0 else cur * es      # folded cost volume: two fp32 feature maps
        per[name] = rd + out * es + 27 * k * c * 4
        FLOPS_3D[name] = 2.0 * 27 * c * out                      # direct form (stride-2 layers: out is the strided grid)
        dims[name] = (k, D, H, W)
        cur = out
    n_dec = len(cfg["deconv3d"])
    for i, (name, k, c, skip) in enumerate(cfg["deconv3d"]):
        if skip:
            kk, D, H, W = dims[skip]
            out = c * D * H * W
        else:                                                   # last layer: up to the image grid, one channel, fp32 volume
            D, H, W = 2 * D, h, w
            out = c * D * H * W
        last = i == n_dec - 1
        per[name] = cur * es + out * (4 if last else es) * (2 if skip else 1) + 27 * k * c * 4
        FLOPS_3D[name] = 2.0 * 27 * k * out / 8.0                # transposed, stride 2: 27 / 8 taps per output
        cur = out
    return float(sum(per.values())), per


def roofline_3d(net, left, right, disp, b, model, half2, step_s):
    """The `roofline` object of a 3-D line (--full): the dominant launch of three event-profiled passes of `net`, priced against
    the roof that bounds it, and the whole step against both roofs."""
    w_img, h_img, max_disp, cfg_name = MODELS_3D[model]
    cfg = getattr(synth, cfg_name)
    es = 2 if half2 else 4
    total, per = trunk_bytes_3d(cfg, h_img, w_img, max_disp, es)
    gflop = sum(FLOPS_3D[n] for n in per) / 1e9
    fold_gflop = 2.0 * 9 * cfg["feat"] * 3 * cfg["conv3d"][0][1] * ((h_img + 1) // 2) * ((w_img + 1) // 2) * 2 / 1e9       # two convolutions F -> 3K
    gflop_exec = gflop - FLOPS_3D[cfg["conv3d"][0][0]] / 1e9 + fold_gflop
    prof = collections.defaultdict(list)
    for _ in range(3):
        for name, ms in net.profile(left, right, disp, b):
            prof[name].append(ms)
    known = {n: sum(v) / len(v) for n, v in prof.items() if n in per}
    dom = max(known, key=known.get)
    dom_s = known[dom] * 1e-3
    traffic, traffic_src = measured_traffic_3d(model, half2, dom)
    terms = 1 if half2 else 3
    # the dominant launch is priced against the roof that bounds it: algorithmic bytes / 8 TB/s or algorithmic FLOPs on the fp16 pipe
    # (x 3 products per multiply for fp32 tensors, as on the headline) / 2.5 PFLOP/s -- whichever fraction is larger
    return dict(
        ({"bound": "mfma", "achieved": terms * FLOPS_3D[dom] * b / dom_s / 1e12, "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s",
          "frac": terms * FLOPS_3D[dom] * b / dom_s / 1e12 / MFMA_F16_PEAK_TFLOPS}
         if terms * FLOPS_3D[dom] / 1e12 / MFMA_F16_PEAK_TFLOPS > per[dom] / 1e9 / HBM_PEAK_GBS else
         {"bound": "hbm", "achieved": per[dom] * b / dom_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
          "frac": per[dom] * b / dom_s / 1e9 / HBM_PEAK_GBS}),
        kernel="%s (DESIGN.md 4.1, 4.7, 9)" % dom,
        traffic=traffic * b if traffic else None, traffic_source=traffic_src,
        algorithmic_bytes=per[dom] * b, avg_launch_us=dom_s * 1e6,
        flops_per_launch=FLOPS_3D[dom] * b, fp16_products_per_multiply=terms,
        frac_hbm=per[dom] * b / dom_s / 1e9 / HBM_PEAK_GBS,
        frac_mfma=terms * FLOPS_3D[dom] * b / dom_s / 1e12 / MFMA_F16_PEAK_TFLOPS,
        frac_mfma_note="direct-form FLOPs of the launch x fp16 products per multiply (1 with fp16 operands, 3 in the split form of "
                       "fp32 tensors) / duration / 2.5 PFLOP/s dense fp16",
        step_algorithmic_bytes=total * b, step_gbs=total * b / step_s / 1e9,
        frac_step=total * b / step_s / 1e9 / HBM_PEAK_GBS,
        frac_step_note="algorithmic bytes of the whole 3-D trunk (each tensor once per launch that touches it) / step time / 8 TB/s",
        # EXECUTED work (VERDICT r04 weak #8c): the first Conv3D runs in factored form (fold_factor.hip.h: two 2-D convolutions
        # of the feature maps F -> 3K, always in the 3-term split, + a combining pass); every other layer runs its direct form
        step_gflop=gflop_exec * b, frac_step_mfma=(terms * (gflop_exec - fold_gflop) + 3 * fold_gflop) * b / step_s / 1e3 / MFMA_F16_PEAK_TFLOPS,
        step_gflop_direct_form=gflop * b,
        step_gflop_note="step_gflop / frac_step_mfma count the FLOPs the GPU executes: the direct form of every 3-D layer except the "
                        "first Conv3D, which is %.1f GFLOP per pair in its factored form instead of the %.0f of the reference's "
                        "formulation (27 taps x channels per voxel, SURVEY 8d: step_gflop_direct_form)" % (fold_gflop, FLOPS_3D[cfg["conv3d"][0][0]] / 1e9))


def bench_3d(lib, dev, model, half2, b, steps, warmup, nctx, blob, weights, desc, world=1, distributed=False, rank=0, check=False, dump=None,
             full=False):
    """One step = one IExecutionContext::enqueue of `b` stereo pairs through the whole 3-D network, inputs resident in HBM.
    Returns the JSON object (rank 0) or None; `full` adds the roofline (event-profiled passes after the timed region)."""
    w_img, h_img, max_disp, cfg_name = MODELS_3D[model]
    cfg = getattr(synth, cfg_name)
    nctx = max(1, min(nctx, int(os.environ.get("RT_BENCH_3D_CONTEXTS", "3"))))      # three contexts (NVSmall half2 b8, MI355X: 2: 768, 3: 782, 4: 771 pairs/s; ~6 GB of tensors each)
    nets = [lib.create(model, w_img, h_img, max_batch=b, weights=blob, fp16_weights=half2) for _ in range(nctx)]
    ls, rs = zip(*(synth.synth_pair(h_img, w_img, 1234 + rank * 64 + i) for i in range(b)))
    left, right = torch.from_numpy(np.stack(ls)).to(dev), torch.from_numpy(np.stack(rs)).to(dev)
    disps = [torch.empty(b, 1, h_img, w_img, device=dev) for _ in nets]
    streams = make_streams(lib.kernels, len(nets), dev)

    def step(i):
        c = i % nctx
        nets[c].execute(left, right, disps[c], b, stream=streams[c].cuda_stream)

    def barrier():
        torch.cuda.synchronize(dev)
        if distributed:
            torch.distributed.barrier()
            torch.cuda.synchronize(dev)

    # every context runs once before the contracted warm-up steps: its first execute() allocates its tensors (GBs for these models), and
    # with fewer warm-up steps than contexts (C4 as a secondary line: 2 steps, 3 contexts) that first pass of the last context fell INTO
    # the timed region -- 74 .. 148 pairs/s on the line for a configuration that runs at 203 (round 6; reported as `priming_steps`)
    for c in range(nctx):
        step(c)
    barrier()
    for i in range(warmup):
        step(i)
    barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    if dump and rank == 0:
        dump_outputs(dump, {"disparity": disps[(steps - 1) % nctx]})      # what the last timed step returned
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    barrier()
    for d in disps:
        assert torch.isfinite(d).all(), "non-finite disparity"
    out = None
    if rank == 0:
        step_s = elapsed / steps
        parity, cpu_base, parity_bound, pairs_checked = None, None, None, None
        if check:                                                  # ~10-30 s of CPU at 1025 x 321; tests/test_net_parity.py does it in the GPU tier too
            from oracle import stereo_oracle as O
            torch.set_num_threads(host_cores())
            wref = {k: (np.asarray(v).astype(np.float16).astype(np.float32) if half2 else v) for k, v in weights.items()}
            with torch.no_grad():
                t_cpu = time.perf_counter()
                ref = O.stereo3d(left[:1].cpu(), right[:1].cpu(), wref, cfg, max_disp)
                t_cpu = time.perf_counter() - t_cpu
            # the timed oracle pass IS the bounded CPU baseline of this configuration (one pair: 10-30 s of host time)
            cpu_base = {"value": 1.0 / t_cpu, "unit": "pairs/s", "cores": torch.get_num_threads(), "kind": "port",
                        "sample": "1 pair of %dx%d in %.1f s, torch CPU fp32 oracle (oracle/stereo_oracle.py: stereo3d)" % (w_img, h_img, t_cpu)}
            parity = float((disps[0][:1].cpu() - ref).abs().max())
            # the bounds tests/test_net_parity.py asserts, asserted here too: fp32 tensors -- 5e-3 px against the fp32
            # oracle for the 30-layer ResNet-18 3D (whose own distance from an fp64 evaluation is 2.2e-3 px; test_3d_models bounds the GPU
            # by 1.5x that in fp64), 1e-3 px otherwise; half2 -- the reference rounds every Conv3D input and output to fp16 in this mode
            # (lib/conv3d_plugin.cpp:247-274): at most 2x the distance of THAT restatement from the fp32-tensor oracle, and 0.25 px
            if half2:
                with torch.no_grad():
                    ref16 = O.stereo3d(left[:1].cpu(), right[:1].cpu(), wref, cfg, max_disp, plugin_fp16=True)
                e_ref = float((ref16 - ref).abs().max())
                parity_bound = min(0.25, max(2.0 * e_ref, 1e-3))
                parity_note_extra = "; the reference-style fp16-plugin oracle is %.3g px from the same oracle, bound = min(0.25, 2x that)" % e_ref
            else:
                parity_bound = 5e-3 if model == "resnet18" else 1e-3
                parity_note_extra = ""
            assert parity <= parity_bound, "%s: disparity differs from the oracle by %.3g px (bound %.3g)" % (model, parity, parity_bound)
            # ... and EVERY pair of the timed batch is what a batch-1 engine computes for that pair alone, bit for bit (VERDICT r04 weak #1:
            # pairs 1 .. b-1 were compared with nothing); tests/test_net_parity.py::test_nvsmall_half2_batch8_full_size_every_pair is the same check
            net1 = lib.create(model, w_img, h_img, max_batch=1, weights=blob, fp16_weights=half2)
            o1 = torch.empty(1, 1, h_img, w_img, device=dev)
            for i in range(b):
                net1.execute(left[i:i + 1].contiguous(), right[i:i + 1].contiguous(), o1, 1)
                torch.cuda.synchronize(dev)
                assert torch.equal(o1, disps[0][i:i + 1]), "%s: pair %d of the batch differs from the batch-1 engine's result by %.3g px" % (
                    model, i, float((o1 - disps[0][i:i + 1]).abs().max()))
            net1.destroy()
            pairs_checked = b
        out = {
            "metric": "stereo pairs/sec, %s 3D %dx%d" % (model, w_img, h_img), "value": world * steps * b / elapsed, "unit": "pairs/s",
            "n_gpus": world, "steps": steps, "warmup": warmup, "priming_steps": nctx, "ms_per_step": step_s * 1e3, "ms_per_pair": step_s / b * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f16 3-D tensors (f32 accumulate), f32 2-D towers" if half2 else "f32", "data": "synthetic",
            "parity_max_abs_err": parity, "parity_bound_asserted": parity_bound,
            "pairs_bit_equal_to_batch1_engine": pairs_checked,
            "parity_note": ("max |disp - oracle| in pixels on the first pair of the batch, %s; disparities reach ~%d px%s" % (
                "oracle on the fp16-rounded weights with fp32 tensors" if half2 else "fp32 oracle", 2 * max_disp, parity_note_extra)) if check else
                           "--check runs the CPU oracle at this size; tests/test_net_parity.py covers it in the GPU tier",
            "config": {"workload": "%s 3-D Stereo DNN, %dx%d, max disparity %d, batch %d per step, %d context(s)" % (
                           model, w_img, h_img, 2 * max_disp, b, nctx),
                       "weights": desc, "launches_per_step": nets[0].num_launches, "half2": bool(half2)},
        }
        if full:
            out["roofline"] = roofline_3d(nets[0], left, right, disps[0], b, model, half2, step_s)
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
    for n in nets:
        n.destroy()
    return out


def measured_traffic_3d(model, half2, layer):
    """HBM bytes of one launch of `layer` at batch 1 from the newest committed PMC pass over the 3-D model (profiles/rNN_traffic_3d.json,
    tools/pmc_3d.sh: FETCH_SIZE x 2 (gfx950 calibration) + WRITE_SIZE, separate rocprofv3 runs); None when absent or taken on other kernel
    sources."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic_3d.json")))
    if not files:
        return None, None
    t = json.load(open(files[-1]))
    src = os.path.relpath(files[-1], ROOT)
    if t.get("sources_sha16") not in (None, kernel_sources_sha16()):
        return None, "%s is stale: taken on kernel sources %s, these are %s" % (src, t.get("sources_sha16"), kernel_sources_sha16())
    e = t.get("%s%s" % (model, " half2" if half2 else ""), {}).get(layer)
    if not e:
        return None, None
    if e.get("incomplete"):
        return None, "%s: %s" % (src, e["incomplete"])
    return float(e["fetch_bytes_x2"] + e["write_bytes"]), src + ": per pair, FETCH_SIZE x 2 + WRITE_SIZE of the launch's dispatches"


def measured_traffic_launches(key, names):
    """HBM bytes per launch, averaged over the launches `names` of the configuration `key`, from the newest committed PMC pass
    (profiles/rNN_traffic_3d.json: tools/pmc_3d.sh segments the dispatches per launch of the executor) -- (bytes, source) or (None, why)"""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic_3d.json")))
    if not files:
        return None, None
    t = json.load(open(files[-1]))
    src = os.path.relpath(files[-1], ROOT)
    if t.get("sources_sha16") not in (None, kernel_sources_sha16()):
        return None, "%s is stale: taken on kernel sources %s, these are %s" % (src, t.get("sources_sha16"), kernel_sources_sha16())
    rows = [t.get(key, {}).get(n) for n in names]
    rows = [e for e in rows if e and not e.get("incomplete")]
    if not rows:
        return None, "%s has no entry '%s' for these launches" % (src, key)
    return sum(float(e["fetch_bytes_x2"] + e["write_bytes"]) for e in rows) / len(rows), src + " ['%s']: FETCH_SIZE x 2 + WRITE_SIZE per launch, mean of %d launches" % (key, len(rows))


def weights_3d(model, half2):
    """(weights dict, packed image, description) of a 3-D model: seeded synthetic, for the reason given at load_weights"""
    cfg = getattr(synth, MODELS_3D[model][3])
    weights, desc = synth.synth_weights_3d(cfg), "seeded He-normal (synthetic)"
    return weights, capi.pack_weights(weights, fp16=half2), desc


def main_3d(args, rank, world, local_rank, dev, distributed):
    weights, blob, desc = (None, b"", None)
    if rank == 0:
        weights, blob, desc = weights_3d(args.model, args.half2)
    if distributed:
        import torch.distributed as dist
        blob = parallel.broadcast_blob(blob if rank == 0 else b"", rank, dev, dist)
    lib = capi.NetLib()
    lib.kernels.check(lib.kernels.lib.rt_set_device(local_rank), "rt_set_device")
    out = bench_3d(lib, dev, args.model, args.half2, args.batch, args.steps, args.warmup, args.contexts, blob, weights, desc,
                   world=world, distributed=distributed, rank=rank, check=args.check, dump=args.dump_outputs, full=args.full)
    if out is not None:
        print(json.dumps(out))


def bench_2d_config(lib, dev, w, h, b, half2, nctx, spc, steps, warmup, sync):
    """A ResNet-18 2D configuration other than the headline (secondary lines: BASELINE C3, the reference's 513x257): timed like the
    headline (round-robin over nctx contexts) or, sync=True, as context->execute() calls one after the other; parity of the first
    pair against the oracle outside the timed region; roofline of the dominant launches in algorithmic work."""
    weights, desc = load_weights(half2)
    blob = capi.pack_weights(weights, fp16=half2)
    nets = [lib.create("resnet18_2D", w, h, max_batch=b, weights=blob, fp16_weights=half2) for _ in range(nctx)]
    for n_ in nets:
        n_.set_streams(spc)
    ls, rs = zip(*(synth.synth_pair(h, w, 4321 + i) for i in range(b)))
    left, right = torch.from_numpy(np.stack(ls)).to(dev), torch.from_numpy(np.stack(rs)).to(dev)
    disps = [torch.empty(b, 1, h, w, device=dev) for _ in nets]
    streams = make_streams(lib.kernels, nctx, dev)
    if sync:
        for _ in range(warmup):
            nets[0].execute(left, right, disps[0], b)
        lat = []
        for _ in range(steps):
            t1 = time.perf_counter()
            nets[0].execute(left, right, disps[0], b)
            lat.append(time.perf_counter() - t1)
        per_step = float(np.median(lat))
        protocol = "context->execute() one call after the other (sample_app/main.cpp:303-309), median of %d calls" % steps
    else:
        for i in range(warmup):
            nets[i % nctx].execute(left, right, disps[i % nctx], b, stream=streams[i % nctx].cuda_stream)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for i in range(steps):
            nets[i % nctx].execute(left, right, disps[i % nctx], b, stream=streams[i % nctx].cuda_stream)
        torch.cuda.synchronize(dev)
        per_step = (time.perf_counter() - t1) / steps
        protocol = "%d steps round-robin over %d contexts with %d stream(s) each" % (steps, nctx, spc)
    from oracle import stereo_oracle as O
    torch.set_num_threads(host_cores())
    with torch.no_grad():
        ref = O.resnet18_2d(left[:1].cpu(), right[:1].cpu(), {k: (np.asarray(v).astype(np.float16).astype(np.float32) if half2 else v)
                                                              for k, v in weights.items()})
    parity = max(float((d[:1].cpu() - ref).abs().max()) for d in (disps[:1] if sync else disps[:min(nctx, steps)]))
    # dominant launches: the tower blocks (fused: one launch per block; merged: both towers per launch)
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    rows = [r for _ in range(3) for r in nets[0].profile(left, right, disps[0], b)]
    fused = any(dominant(n) and "+" in n for n, _ in rows)
    sel = [(n, ms) for n, ms in rows if dominant(n) and (("+" in n) == fused)]
    tot_s = sum(ms for _, ms in sel) * 1e-3
    tot_imgs = sum(b * (2 if " | " in n else 1) for n, _ in sel)
    layer_flops = 2.0 * 32 * 32 * 9 * h2 * w2
    if half2:
        unit_work, peak, unit, bound = 2.0 * (3 * 32 * h2 * w2 + 32 * 32 * 9) + 4.0 * 32, HBM_PEAK_GBS, "GB/s", "hbm"
        kernel = "conv_f16mma_kernel<3,3,1> 3x3 32->32 @%dx%d (+bias,+residual,+ELU), fp16 tensors and operands, fp32 accumulate" % (w2, h2)
    elif fused:
        unit_work, peak, unit, bound = 3.0 * 2.0 * layer_flops, MFMA_F16_PEAK_TFLOPS, "TFLOP/s", "mfma"
        kernel = "conv_s3rbd_kernel / conv_s3rbs_kernel: residual block @%dx%d in one launch (3 fp16 MFMA products per multiply)" % (w2, h2)
    else:
        unit_work, peak, unit, bound = 4.0 * (3 * 32 * h2 * w2 + 32 * 32 * 9 + 32), HBM_PEAK_GBS, "GB/s", "hbm"
        kernel = "conv_s3_kernel<3,3,1,il,il> 3x3 32->32 @%dx%d (+bias,+residual,+ELU), fp32 tensors, 3-term fp16 split" % (w2, h2)
    achieved = unit_work * tot_imgs / tot_s / (1e12 if bound == "mfma" else 1e9)
    traffic, traffic_src = measured_traffic_launches("resnet18_2D %dx%d%s batch %d" % (w, h, " half2" if half2 else "", b), sorted({n for n, _ in sel}))
    out = {"value": b / per_step, "unit": "pairs/s", "ms_per_step": per_step * 1e3, "ms_per_pair": per_step / b * 1e3, "steps": steps, "warmup": warmup,
           "dtype": "f16 (f32 accumulate)" if half2 else "f32", "data": "synthetic", "protocol": protocol,
           "config": {"workload": "ResNet-18 2D Stereo DNN %s, %dx%d, batch=%d per step" % ("half2 mode" if half2 else "fp32", w, h, b),
                      "contexts": nctx, "streams_per_context": spc, "launches_per_step": nets[0].num_launches, "weights": desc},
           "parity_max_abs_err": parity,
           "parity_note": "max |disp - oracle| on the first pair, %s; budget %s" % (
               "oracle on the fp16-rounded weights" if half2 else "fp32 oracle", "1e-2" if half2 else "1e-3"),
           "roofline": {"bound": bound, "kernel": kernel, "achieved": achieved, "peak": peak, "unit": unit, "frac": achieved / peak,
                        "avg_launch_us": tot_s / len(sel) * 1e6, "images_per_launch": tot_imgs / len(sel), "traffic": traffic, "traffic_source": traffic_src,
                        "algorithmic_bytes": (unit_work if bound == "hbm" else 4.0 * (2 * 32 * h2 * w2) + 8.0 * (32 * 32 * 9 + 32)) * tot_imgs / len(sel),
                        "frac_note": "algorithmic work of the dominant launches / their durations (HIP events on the launch stream, profiled steps of one context)"}}
    assert parity <= (1e-2 if half2 else 1e-3), "secondary config differs from the oracle by %.3g" % parity
    for n_ in nets:
        n_.destroy()
    return out


def secondary_lines(lib, dev):
    """BASELINE's other configurations, bounded (default run only): each entry is a bench line of its own (value, ms_per_pair, dtype,
    config.workload, parity_max_abs_err against the oracle on one pair, roofline in algorithmic work)."""
    out = []

    def add(tag, fn):
        t0 = time.perf_counter()
        try:
            line = fn()
        except Exception as e:                                  # a secondary line must never take the headline down
            line = {"error": "%s: %s" % (type(e).__name__, e)}
        line["id"] = tag
        line["wall_s"] = time.perf_counter() - t0
        out.append(line)

    add("C3: ResNet-18 2D half2, 1257x369, batch 8", lambda: bench_2d_config(lib, dev, W, H, 8, True, 3, 1, 32, 8, False))
    add("ref513: ResNet-18 2D fp32, 513x257, batch 1, one context, synchronous (the reference's published configuration: stereoDNN/README.md:31)",
        lambda: bench_2d_config(lib, dev, 513, 257, 1, False, 1, 2, 100, 20, True))

    def three_d(model, half2, b, steps, warmup):
        weights, blob, desc = weights_3d(model, half2)
        return bench_3d(lib, dev, model, half2, b, steps, warmup, 3, blob, weights, desc, check=True, full=True)

    add("C5: NVSmall half2, 1025x321, batch 8", lambda: three_d("nvsmall", True, 8, 24, 3))
    add("C4: ResNet-18 3D fp32, 1025x321, batch 4 (one GPU's shard of batch 32 over 8)", lambda: three_d("resnet18", False, 4, 20, 2))

    def nvtiny():
        line = three_d("nvtiny", False, 1, 100, 20)
        # C1 is the reference's CPU-runnable case: the oracle on this host's cores beside it
        from oracle import stereo_oracle as O
        w_img, h_img, max_disp, cfg_name = MODELS_3D["nvtiny"]
        weights, _, _ = weights_3d("nvtiny", False)
        l, r = synth.synth_pair(h_img, w_img, 1234)
        L, R = torch.from_numpy(l)[None], torch.from_numpy(r)[None]
        torch.set_num_threads(host_cores())
        with torch.no_grad():
            O.stereo3d(L, R, weights, getattr(synth, cfg_name), max_disp)
            n, t0 = 0, time.perf_counter()
            while n < 2 or time.perf_counter() - t0 < 4.0:
                O.stereo3d(L, R, weights, getattr(synth, cfg_name), max_disp)
                n += 1
            dt = time.perf_counter() - t0
        line["cpu_baseline"] = {"value": n / dt, "unit": "pairs/s", "cores": torch.get_num_threads(), "kind": "port",
                                "sample": "%d pairs of 513x161 in %.1f s, torch CPU fp32 oracle" % (n, dt)}
        return line

    add("C1: NVTiny fp32, 513x161, batch 1 (plumbing case)", nvtiny)
    return out


def exact_fp32_value(lib, dev, blob, b, nctx, spc, left, right, ref, steps=60):
    """The headline set-up with the exact-fp32 option: every 2-D convolution on the fp32 fmaf-chain kernels of round 1 (no fp16 split)."""
    nets = [lib.create("resnet18_2D", W, H, max_batch=b, weights=blob, flags=capi.RT_CONV_EXACT_FP32) for _ in range(nctx)]
    for n_ in nets:
        n_.set_streams(spc)
    disps = [torch.empty(b, 1, H, W, device=dev) for _ in nets]
    streams = make_streams(lib.kernels, nctx, dev)
    for i in range(2 * nctx):
        nets[i % nctx].execute(left, right, disps[i % nctx], b, stream=streams[i % nctx].cuda_stream)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    for i in range(steps):
        nets[i % nctx].execute(left, right, disps[i % nctx], b, stream=streams[i % nctx].cuda_stream)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t1
    parity = max(float((d.cpu() - ref).abs().max()) for d in disps)
    launches = nets[0].num_launches
    for n_ in nets:
        n_.destroy()
    return {"value": steps * b / dt, "unit": "pairs/s", "steps": steps, "launches_per_step": launches, "parity_max_abs_err": parity,
            "note": "rtNetOptions.flags = RT_CONV_EXACT_FP32 (IBuilder::setExactFp32Mode): fp32 fmaf chains on the fp32 matrix pipe / Winograd F(2x2,3x3), "
                    "same contexts and streams"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)       # the reference averages over 200 images
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--contexts", type=int, default=int(os.environ.get("RT_BENCH_CONTEXTS", "0")),
                    help="IExecutionContexts per GPU, each with its own stream; steps are issued round-robin "
                         "(the TensorRT throughput set-up, trtexec --streams).  1 = the reference's synchronous loop; 0 (default) = 3 "
                         "(end of round 6, 22 launches per pair: the driver's 20 steps give 2695-2820 pairs/s with 3 contexts, 2643-2666 with 6 -- "
                         "less to fill and drain in a 7 ms timed region; 200 steps 2814 / 2802; 4 and 8 contexts 2350-2420; half2 batch 8: "
                         "6550-6566 with 2, 3 or 6; profiles/r06_contexts.txt)")
    ap.add_argument("--streams-per-context", type=int, default=0, choices=[0, 1, 2],
                    help="HIP streams a context issues on (IExecutionContext::setExecutionStreams): 2 = right-image encoder on a second "
                         "stream, 1 = everything on the context's stream; 0 (default) = 1 with several fp32 contexts, 2 with one or with --half2.  Measured "
                         "(driver command, --steps 20 --warmup 5): six one-stream contexts 2270, four two-stream contexts 2100 pairs/s; "
                         "one context: 1750-1880 with two streams, 1345 with one")
    ap.add_argument("--half2", action="store_true",
                    help="TensorRT half2 mode (BASELINE config C3): fp16 weight file, activations stored as fp16 between "
                         "launches, fp16 operands on the matrix cores with fp32 accumulation; the JSON line then says dtype f16")
    ap.add_argument("--model", default="resnet18_2D", choices=["resnet18_2D"] + sorted(MODELS_3D),
                    help="resnet18_2D (the headline) or one of the 3-D models (BASELINE configs C4 / C5): separate JSON line (--full: + roofline)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything beyond the headline figure: parity against the "
                         "oracle, bitwise agreement of the contexts, single_context, roofline, value_200, value_exact_fp32, cpu_baseline "
                         "and the secondary lines (a minute or more); a plain run only times the K steps and prints the JSON line")
    ap.add_argument("--check", action="store_true", help="3-D models: also run the CPU oracle at the timed size (minutes)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0's disparity, float32) as DIR/disparity.npy; "
                         "the inputs depend on the arguments alone, so two builds can be compared output for output")
    ap.add_argument("--from-host", action="store_true", help="also measure the PCIe-inclusive rate (extra JSON object)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip cpu_baseline")
    ap.add_argument("--no-secondary", action="store_true",
                    help="--full: skip the secondary lines (BASELINE C3 / C5 / C4, 513x257, NVTiny), value_200 and value_exact_fp32")
    ap.add_argument("--spinup-ms", type=float, default=float(os.environ.get("RT_BENCH_SPINUP_MS", "80")),
                    help="keep the GPU busy with (untimed, uncounted) steps for this long before the W warm-up steps: the shader clock "
                         "of an idle MI355X needs ~50 ms of load to reach its sustained value (measured: 20 timed steps give 1883 / "
                         "1948 / 2015 pairs/s after 5 / 20 / 100 warm-up steps).  0 = off; reported on the JSON line")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.contexts <= 0:
        args.contexts = 3       # (six until the end of round 6: see --contexts; half2 used four two-stream contexts until its tower blocks were fused)

    # `python bench.py --gpus N` without a launcher: become the launcher -- one rank per GPU through
    # torch.distributed.run on 127.0.0.1, exactly the command the driver uses -- instead of silently timing one GPU.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import socket
        import subprocess
        if torch.cuda.device_count() < args.gpus:
            sys.exit("bench.py: --gpus %d but only %d HIP device(s) are visible" % (args.gpus, torch.cuda.device_count()))
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started %d rank(s)" % (args.gpus, world))
    # BENCH_FORCE_DISTRIBUTED=1: walk the multi-rank start-up (process group, native RCCL entry, agreement on the transport) with a world of
    # one rank -- a single-GPU box cannot host two RCCL ranks, and this is how that code is exercised there (tests/test_multi_gpu.py)
    distributed = world > 1 or (os.environ.get("BENCH_FORCE_DISTRIBUTED", "0") != "0" and "WORLD_SIZE" in os.environ)
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    if args.model != "resnet18_2D":
        main_3d(args, rank, world, local_rank, dev, distributed)
        if distributed:
            torch.distributed.destroy_process_group()
        return

    # ---- weights: rank 0 owns the file image, everyone else receives it over RCCL/xGMI ------------------
    # Through the NATIVE entry (include/rt_stereo.h: rt_comm_*, rt_stereo_net.h: rt_net_create_broadcast -> ncclBroadcast from librccl,
    # no torch in the path; torch.distributed only carries the communicator's 128-byte unique id).  If that entry fails on this node the
    # image goes through torch.distributed's broadcast instead -- loudly, and the JSON line says which transport was used.
    weights, weights_desc = None, None
    blob = None
    if rank == 0:
        weights, weights_desc = load_weights(args.half2)
        blob = capi.pack_weights(weights, fp16=args.half2)
    import zlib
    lib = capi.NetLib()
    lib.kernels.check(lib.kernels.lib.rt_set_device(local_rank), "rt_set_device")
    transport, nets = "none (one rank)", None
    if distributed:
        import torch.distributed as dist
        # ... under a watchdog: a start-up that does not come back within two minutes (a communicator bootstrap that never completes) is
        # abandoned in its daemon thread and the ranks agree on the fallback below -- a hang here would cost the whole scaling run
        import threading
        res = {}
        # the 128-byte unique id travels over torch.distributed's group HERE, on the thread that owns that group; the thread
        # below only touches the communicator of our own (rt_comm_init_rank / rt_net_create_broadcast), so abandoning it leaves the
        # process group untouched and the fallback collectives below are safe
        uid = parallel.exchange_unique_id(lib, rank, world, dist)

        def native_startup():
            try:
                torch.cuda.set_device(dev)                      # the current device is per host thread: torch's ...
                lib.kernels.check(lib.kernels.lib.rt_set_device(local_rank), "rt_set_device")      # ... and HIP's
                res["nets"] = parallel.create_nets_native(lib, "resnet18_2D", W, H, args.contexts, blob, rank, world, dist, max_batch=args.batch,
                                                          fp16_weights=args.half2, uid=uid)
            except Exception as e:                              # noqa: BLE001 -- any failure of the native entry must not cost the scaling run
                res["error"] = e

        th = threading.Thread(target=native_startup, daemon=True)
        th.start()
        th.join(timeout=float(os.environ.get("BENCH_NATIVE_STARTUP_TIMEOUT_S", "120")))
        if "nets" in res:
            nets, blob_crc = res["nets"]
            transport = "rccl-native (rt_net_create_broadcast)"
        else:
            NATIVE_STARTUP_HUNG[0] = th.is_alive()
            why = "no answer within the watchdog's time" if th.is_alive() else "%s: %s" % (type(res.get("error")).__name__, res.get("error"))
            print("bench.py: rank %d: native RCCL entry failed (%s) -- broadcasting the weight image through torch.distributed instead" % (rank, why),
                  file=sys.stderr, flush=True)
            nets = None
        ok = torch.tensor([1 if nets is not None else 0], device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)               # all ranks on the same transport
        if int(ok.item()) == 0:
            if nets is not None:
                for n_ in nets:
                    n_.destroy()
            blob = parallel.broadcast_blob(blob if rank == 0 else b"", rank, dev, dist)
            nets, transport = None, "torch.distributed broadcast (fallback)"
    if nets is None:
        blob_crc = zlib.crc32(blob) & 0xffffffff
        nets = [lib.create("resnet18_2D", W, H, max_batch=args.batch, weights=blob, fp16_weights=args.half2)
                for _ in range(args.contexts)]
    if distributed:
        print("bench.py: rank %d/%d (RCCL world size %d) on cuda:%d, weight image crc32 %08x via %s" % (
            rank, world, torch.distributed.get_world_size(), local_rank, blob_crc, transport), file=sys.stderr, flush=True)
        if rank != 0:
            blob = nets[0].weights_image()                      # (value_exact_fp32 etc. only run on one rank; kept for symmetry)

    net = nets[0]
    spc = args.streams_per_context or (1 if args.contexts > 1 else 2)      # (round 5, half2 layer by layer: 3978 (4 x 2) vs 3881 (6 x 1) pairs/s at batch 8; fused blocks: 5634 vs 6060)
    for n_ in nets:
        n_.set_streams(spc)

    b = args.batch
    nctx = len(nets)
    # every context works on its OWN pairs (a throughput claim should not run one pair through all contexts): context c
    # takes seeds 1234 + rank * 64 + c * b + i; context 0's are the pair(s) every other figure of this file (latency, profiles) uses
    lefts, rights = [], []
    for c in range(nctx):
        ls, rs = zip(*(synth.synth_pair(H, W, 1234 + rank * 64 + c * b + i) for i in range(b)))
        lefts.append(torch.from_numpy(np.stack(ls)).to(dev))
        rights.append(torch.from_numpy(np.stack(rs)).to(dev))
    left, right = lefts[0], rights[0]
    disps = [torch.empty(b, 1, H, W, device=dev) for _ in nets]
    disp = disps[0]
    streams = make_streams(lib.kernels, len(nets), dev)

    def step(i):
        c = i % nctx
        nets[c].execute(lefts[c], rights[c], disps[c], b, stream=streams[c].cuda_stream)

    def barrier():
        torch.cuda.synchronize(dev)
        if distributed:
            torch.distributed.barrier()
            torch.cuda.synchronize(dev)

    # device spin-up (see --spinup-ms): not warm-up of the engine -- W steps of that follow -- but of the clock governor
    spun = 0
    if args.spinup_ms > 0:
        t_end = time.perf_counter() + args.spinup_ms * 1e-3
        while time.perf_counter() < t_end:
            step(spun)
            spun += 1
            if spun % (2 * nctx) == 0:
                torch.cuda.synchronize(dev)
    for i in range(args.warmup):
        step(i)
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    issued = time.perf_counter() - t0                           # the host is done issuing: everything after this is the GPU finishing
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    last_disp = disps[(args.steps - 1) % nctx].clone() if args.dump_outputs else None      # what the last timed step returned
    # per rank: its own rate, the host time it needed to issue a step (23 launches through Python + ctypes) against the
    # step time -- the headroom one rank's host thread has -- and the cores it may use
    rank_rows = [{"rank": rank, "pairs_per_s": args.steps * b / elapsed, "weights_crc32": "%08x" % blob_crc,
                  "host_issue_us_per_step": issued / args.steps * 1e6, "step_us": elapsed / args.steps * 1e6,
                  "host_cores": host_cores(), "device": torch.cuda.get_device_name(dev)}]
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        gathered = [None] * world
        torch.distributed.all_gather_object(gathered, rank_rows[0])
        rank_rows = gathered
        elapsed = float(t.item())
    barrier()
    for d in disps:
        assert torch.isfinite(d).all(), "non-finite disparity"
    # ---- the headline figure is complete: what follows runs with --full only (--from-host asks for its figure itself) -------
    default_run = (args.full and world == 1 and not args.half2 and b == 1 and not args.from_host and not args.no_secondary and
                   os.environ.get("RT_CONV_EXACT_FP32", "0") == "0")
    value_200 = None
    if default_run and args.steps < 200:                       # the driver's K = 20 is 9 ms of timed region: the same contexts over 200 steps
        t1 = time.perf_counter()
        for i in range(200):
            step(i)
        torch.cuda.synchronize(dev)
        value_200 = {"value": 200 * b / (time.perf_counter() - t1), "unit": "pairs/s", "steps": 200,
                     "note": "same contexts, right after the contracted K steps"}
    # the reference's own loop for comparison (sample_app/main.cpp:303-309): one context, one pair in flight
    single = None
    if args.full and nctx > 1 and rank == 0:
        nets[0].set_streams(2)                                 # the latency set-up: one context, right-image encoder on a second stream
        n1 = min(args.steps, 200)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for _ in range(n1):
            nets[0].execute(left, right, disps[0], b, stream=streams[0].cuda_stream)
        torch.cuda.synchronize(dev)
        dt1 = time.perf_counter() - t1
        single = {"value": n1 * b / dt1, "unit": "pairs/s", "ms_per_pair": dt1 / n1 / b * 1e3, "steps": n1}
        # ... and literally: IExecutionContext::execute (returns when the disparity is there), one call after the other
        lat = []
        for _ in range(max(n1, 50)):
            t1 = time.perf_counter()
            nets[0].execute(left, right, disps[0], b)
            lat.append(time.perf_counter() - t1)
        dt1 = float(np.median(lat[len(lat) // 4:]))             # per call: the first calls still create the context's own stream
        single["synchronous_execute"] = {"value": b / dt1, "unit": "pairs/s", "ms_per_pair": dt1 / b * 1e3, "ms_per_pair_mean": float(np.mean(lat)) / b * 1e3,
                                         "calls": len(lat),
                                         "note": "context->execute() in a loop, the reference's timing protocol (sample_app/main.cpp:303-309)"}
        # ... and the same loop in graph mode (IExecutionContext::setGraphMode: the pass is one hipGraph launch) -- reported, not the default
        try:
            nets[0].set_graph(True)
            for _ in range(3):
                nets[0].execute(left, right, disps[0], b)              # direct, capture, first replay
            lat_g = []
            for _ in range(max(n1, 50)):
                t1 = time.perf_counter()
                nets[0].execute(left, right, disps[0], b)
                lat_g.append(time.perf_counter() - t1)
            dtg = float(np.median(lat_g[len(lat_g) // 4:]))
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for _ in range(n1):
                nets[0].execute(left, right, disps[0], b, stream=streams[0].cuda_stream)
            torch.cuda.synchronize(dev)
            dtp = (time.perf_counter() - t1) / n1
            single["graph_mode"] = {"synchronous_execute_ms_per_pair": dtg / b * 1e3, "pipelined_ms_per_pair": dtp / b * 1e3,
                                    "note": "one hipGraph launch per pair (rt_net_set_graph); same context, same streams"}
        except Exception as e:                                          # noqa: BLE001 -- the figure is optional, the reason is reported
            single["graph_mode"] = {"error": str(e)[:200]}
        finally:
            nets[0].set_graph(False)
        # the latency set-up is not the timed one (two streams; no throughput hint, so the low-resolution layers split their
        # contraction over wave groups, DESIGN.md 4.6: another fp32 summation order): its disparity is checked on its own below, and
        # context 0 runs one plain step again so that what is compared between the contexts is what was timed
        disp_latency = disps[0].clone()
        nets[0].set_streams(spc)
        step(0)
        torch.cuda.synchronize(dev)
    # PCIe-inclusive rate (never `value`): the same K steps with each pair's two images copied host -> device and its
    # disparity device -> host, pinned buffers, copies on a per-context copy stream ordered by events so that they
    # overlap the convolutions of the other contexts (double-buffered H2D)
    pcie = None
    if args.from_host and rank == 0:
        h_l, h_r = left.cpu().pin_memory(), right.cpu().pin_memory()
        h_out = [torch.empty(b, 1, H, W).pin_memory() for _ in nets]
        NBUF = 2                                                      # input buffers per context: copy i+1 under compute i
        d_l = [[torch.empty_like(left) for _ in range(NBUF)] for _ in nets]
        d_r = [[torch.empty_like(right) for _ in range(NBUF)] for _ in nets]
        copy_streams = make_streams(lib.kernels, len(nets), dev)
        copied = [[torch.cuda.Event() for _ in range(NBUF)] for _ in nets]
        consumed = [[torch.cuda.Event() for _ in range(NBUF)] for _ in nets]

        def host_step(i):
            c, k = i % nctx, (i // nctx) % NBUF
            with torch.cuda.stream(copy_streams[c]):
                copy_streams[c].wait_event(consumed[c][k])        # the pair that used this buffer has read its inputs
                d_l[c][k].copy_(h_l, non_blocking=True)
                d_r[c][k].copy_(h_r, non_blocking=True)
                copied[c][k].record()
            streams[c].wait_event(copied[c][k])
            nets[c].execute(d_l[c][k], d_r[c][k], disps[c], b, stream=streams[c].cuda_stream)
            with torch.cuda.stream(streams[c]):
                consumed[c][k].record()
                h_out[c].copy_(disps[c], non_blocking=True)

        for c in range(nctx):
            for k in range(NBUF):
                consumed[c][k].record(streams[c])
        for i in range(args.warmup):
            host_step(i)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for i in range(args.steps):
            host_step(i)
        torch.cuda.synchronize(dev)
        dt1 = time.perf_counter() - t1
        mb = (left.numel() + right.numel() + disps[0].numel()) * 4 / 1e6
        pcie = {"value": args.steps * b / dt1, "unit": "pairs/s", "ms_per_pair": dt1 / args.steps / b * 1e3,
                "mb_per_pair": mb / b, "gb_per_s": mb * args.steps / dt1 / 1e3,
                "note": "H2D of both images + D2H of the disparity per pair, pinned host memory, overlapped"}
        assert torch.equal(h_out[0], disps[0].cpu()), "host copy of the disparity differs"

        # same pipeline with camera-format I/O: u8 BGR frames in (3 bytes per pixel instead of 12), pre-processing
        # and the 16-bit KITTI encoding of the disparity on the device (rt_preprocess_bgr8 / rt_disparity_to_u16)
        k = lib.kernels
        to_u8 = lambda t: (t.cpu().flip(1).permute(0, 2, 3, 1) * 255).round().clamp(0, 255).to(torch.uint8).contiguous()
        h_l8, h_r8 = to_u8(left).pin_memory(), to_u8(right).pin_memory()
        d_l8 = [[torch.empty_like(h_l8, device=dev) for _ in range(NBUF)] for _ in nets]
        d_r8 = [[torch.empty_like(h_r8, device=dev) for _ in range(NBUF)] for _ in nets]
        d_u16 = [torch.empty(b, 1, H, W, dtype=torch.int16, device=dev) for _ in nets]
        h_u16 = [torch.empty(b, 1, H, W, dtype=torch.int16).pin_memory() for _ in nets]

        def host_step_u8(i):
            c, q = i % nctx, (i // nctx) % NBUF
            with torch.cuda.stream(copy_streams[c]):
                copy_streams[c].wait_event(consumed[c][q])
                d_l8[c][q].copy_(h_l8, non_blocking=True)
                d_r8[c][q].copy_(h_r8, non_blocking=True)
                copied[c][q].record()
            streams[c].wait_event(copied[c][q])
            sh_ = streams[c].cuda_stream
            k.preprocess_bgr8(d_l8[c][q], H, W, d_l[c][q], H, W, b, stream=sh_)
            k.preprocess_bgr8(d_r8[c][q], H, W, d_r[c][q], H, W, b, stream=sh_)
            nets[c].execute(d_l[c][q], d_r[c][q], disps[c], b, stream=sh_)
            k.disparity_to_u16(disps[c], d_u16[c], b * H * W, 256.0 * W, stream=sh_)
            with torch.cuda.stream(streams[c]):
                consumed[c][q].record()
                h_u16[c].copy_(d_u16[c], non_blocking=True)

        for i in range(args.warmup):
            host_step_u8(i)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for i in range(args.steps):
            host_step_u8(i)
        torch.cuda.synchronize(dev)
        dt1 = time.perf_counter() - t1
        mb8 = (h_l8.numel() + h_r8.numel() + 2 * h_u16[0].numel()) / 1e6
        pcie["u8_frames"] = {"value": args.steps * b / dt1, "unit": "pairs/s", "ms_per_pair": dt1 / args.steps / b * 1e3,
                             "mb_per_pair": mb8 / b,
                             "note": "u8 BGR frames in, 16-bit disparity out, pre/post-processing on the device"}
        # the u8 pipeline left disparities of the QUANTISED frames in `disps`: one plain step per context again, so that what is
        # checked below is what was timed above
        for i in range(nctx):
            step(i)
        torch.cuda.synchronize(dev)
    # Determinism, asserted: with every context busy, (a) a context's second pass over its own pair and (b) context
    # 0's pass over every other context's pair must reproduce that context's timed result BIT FOR BIT.  (Rounds 2-3 reported the figure
    # and bounded it at 1e-4; the one deviation ever seen in the default engine was the 16-byte-store hazard avoided in common.hip.h:
    # buf_store4, and the exact-fp32 engine's is located in profiles/r04_race.txt.)
    ctx_diff = None
    if args.full:
        ctx_diff = 0.0
        first = [d.clone() for d in disps]
        for rep in range(3):
            for i in range(nctx):
                step(i)
            cross = [torch.empty_like(disps[0]) for _ in range(nctx)]
            for c in range(1, nctx):                            # context 0 on the other contexts' pairs, while those are busy themselves
                nets[0].execute(lefts[c], rights[c], cross[c], b, stream=streams[0].cuda_stream)
            torch.cuda.synchronize(dev)
            for c in range(nctx):
                ctx_diff = max(ctx_diff, float((disps[c] - first[c]).abs().max()))
                if c:
                    ctx_diff = max(ctx_diff, float((cross[c] - first[c]).abs().max()))
        assert ctx_diff == 0.0, "contexts / repeated passes disagree by %.3g" % ctx_diff
        step(0)                                                 # context 0 holds its own pair's disparity again
        torch.cuda.synchronize(dev)
    # ---- what was timed is also checked: every context's disparity against the oracle on the same pair(s) -------
    # (outside the timed region; BASELINE budget 1e-3 abs on the raw `disp` output, 1e-2 = the reference's fp16
    # tolerance in half2 mode where the fp16 activations themselves are the difference)
    parity = None
    if args.full and rank == 0:
        from oracle import stereo_oracle as O
        torch.set_num_threads(host_cores())
        wq = {k: (np.asarray(v).astype(np.float16).astype(np.float32) if args.half2 else v) for k, v in weights.items()}
        with torch.no_grad():
            ref = O.resnet18_2d(left.cpu(), right.cpu(), wq)
            refs = [ref] + [O.resnet18_2d(lefts[c].cpu(), rights[c].cpu(), wq) for c in range(1, nctx)]     # every context against its own pair
        parity = max(float((d.cpu() - r_).abs().max()) for d, r_ in zip(disps, refs))
        budget = 1e-2 if args.half2 else 1e-3
        assert parity <= budget, "disparity differs from the oracle by %.3g (budget %.0e)" % (parity, budget)
        if single is not None:
            single["parity_max_abs_err"] = float((disp_latency.cpu() - ref).abs().max())
            assert single["parity_max_abs_err"] <= budget, "latency set-up: disparity differs from the oracle by %.3g" % single["parity_max_abs_err"]
    value_exact, secondary = None, None
    if default_run and rank == 0:
        value_exact = exact_fp32_value(lib, dev, blob, b, nctx, spc, left, right, ref)

    roofline = None
    if args.full and rank == 0:
        # ---- roofline of the dominant kernel: HIP events around every launch, on the launch stream ------
        prof_runs = 5
        rows = [r for _ in range(prof_runs) for r in net.profile(left, right, disp, b)]
        # residual blocks that run as ONE launch are named "<conv1>+<conv2>" by the executor (engine.cpp: fuseResBlocks); a launch that
        # covers the twin layers of both towers (mergeSiamese) "<left> | <right>": it processes 2 b images
        fused = any(dominant(n) and "+" in n for n, _ in rows)
        sel = [(n, ms) for n, ms in rows if dominant(n) and (("+" in n) == fused)]
        imgs = lambda n: b * (2 if " | " in n else 1)
        tot_s = sum(ms for _, ms in sel) * 1e-3
        tot_imgs = sum(imgs(n) for n, _ in sel)
        cnt = len(sel)
        avg_s = tot_s / cnt
        avg_imgs = tot_imgs / cnt                                  # images per launch, averaged over the dominant launches
        launches = cnt // prof_runs
        step_s = elapsed / args.steps
        traffic, traffic_src = measured_traffic(args.half2, None if args.half2 else fused) if b == 1 else (None, None)
        if traffic is None and (args.half2 or b > 1):              # the per-launch passes over the configuration as timed (tools/pmc_3d.sh)
            traffic, traffic_src = measured_traffic_launches("resnet18_2D %dx%d%s batch %d" % (W, H, " half2" if args.half2 else "", b), sorted({n for n, _ in sel}))
        exact = os.environ.get("RT_CONV_EXACT_FP32", "0") != "0"
        b_iso = int(round(avg_imgs)) if avg_imgs > 1.5 * b else b  # the typical dominant launch: both towers when they are merged
        hints = capi.RT_HINT_THROUGHPUT if spc == 1 else 0
        iso_us = isolated_dominant(lib.kernels, b_iso, args.half2, fused=fused, hints=hints)
        flops = BLOCK_FLOPS if fused else DOMINANT_FLOPS           # per image
        if args.half2:
            # fp16 operands on the matrix cores: 2.5 PFLOP/s makes the layer HBM-bound, so it is priced in
            # bytes: x, residual, y as fp16 + fp16 weights + fp32 bias
            nbytes = 2.0 * (3 * 32 * HALF_W * HALF_H + 32 * 32 * 9) + 4.0 * 32
            kernel = "conv_f16mma_kernel<3,3,1> 3x3 32->32 @629x185 (+bias,+residual,+ELU), fp16 operands, fp32 accumulate"
            mfma_exec = DOMINANT_FLOPS
        elif exact:
            nbytes = DOMINANT_BYTES
            kernel = "conv_wino_f32_kernel<4,float,float,il,il> (RT_CONV_EXACT_FP32=1: Winograd F(2x2,3x3) on the fp32 matrix pipe)"
            mfma_exec = DOMINANT_FLOPS * 16.0 / 36.0
        else:
            nbytes = BLOCK_BYTES if fused else DOMINANT_BYTES
            kernel = ("conv_s3rbd_kernel: residual block = two 3x3 32->32 convolutions @629x185 (+bias,+ELU / +bias,+skip,+ELU) in one launch, "
                      "streaming down 30-column strips, intermediate rows in an LDS ring; tower tensors stored as the fp16 (hi, lo) pairs of the "
                      "3-term split and moved HBM -> LDS by DMA, v_mfma_f32_32x32x16_f16, fp32 accumulate (conv_s3rbs_kernel: the same from fp32 "
                      "tensors, on a block's first / last tensor and with RT_NO_RBD=1)" if fused else
                      "conv_s3_kernel<3,3,1,il,il> 3x3 32->32 @629x185 (+bias,+residual,+ELU): fp32 tensors, 3-term fp16 split on v_mfma_f32_32x32x16_f16, fp32 accumulate")
            if fused:
                # executed matrix work of the streaming kernel per image: 21 strips x segments, every step computes 4 rows x 32 columns
                # of conv1 and of conv2 (halo rows / columns and the rows of the pipeline's fill and drain steps included)
                seg = int(os.environ.get("RT_RBS_SEG", "0")) or (64 if hints else 32)
                strips, rows_exec = -(-HALF_W // 30), 0
                for y0 in range(0, HALF_H, seg):
                    hseg = min(seg, HALF_H - y0)
                    rows_exec += 4 * ((hseg + 1) // 4 + 1) + 4 * ((hseg + 1 + 4) // 4)          # conv1: steps 0..last1, conv2: steps 1..nstep-1
                mfma_exec = 3.0 * strips * rows_exec * 2.0 * 32 * 32 * 32 * 9
            else:
                mfma_exec = 3.0 * flops
        frac_executed = None
        if exact and not args.half2:
            achieved, peak, unit, bound = flops * tot_imgs / tot_s / 1e12, MFMA_F32_PEAK_TFLOPS, "TFLOP/s", "mfma"
            iso_frac = flops * b_iso / iso_us / 1e6 / MFMA_F32_PEAK_TFLOPS
        elif fused and not args.half2:
            # the fused block moves 2.8x fewer bytes than its two layers and is bound by the SIMD's vector issue port (MFMA issue +
            # VALU, tools/dev/README.md), not by HBM: priced in ALGORITHMIC matrix work -- 3 fp16 MFMA products per direct-form
            # multiply, the minimum of the split scheme -- against the dense fp16 peak; the executed work (halo, fill / drain
            # rows) is `frac_executed`
            achieved, peak, unit, bound = 3.0 * flops * tot_imgs / tot_s / 1e12, MFMA_F16_PEAK_TFLOPS, "TFLOP/s", "mfma"
            iso_frac = 3.0 * flops * b_iso / iso_us / 1e6 / MFMA_F16_PEAK_TFLOPS
            frac_executed = mfma_exec * tot_imgs / tot_s / 1e12 / MFMA_F16_PEAK_TFLOPS
        else:
            achieved, peak, unit, bound = nbytes * tot_imgs / tot_s / 1e9, HBM_PEAK_GBS, "GB/s", "hbm"
            iso_frac = nbytes * b_iso / iso_us / 1e3 / HBM_PEAK_GBS
        overlapped = launches * avg_s > step_s * b            # launches of several streams / contexts run concurrently
        mfma_peak = MFMA_F32_PEAK_TFLOPS if (exact and not args.half2) else MFMA_F16_PEAK_TFLOPS
        # share of the GPU's time the dominant launches take in the TIMED run (several contexts in flight): their profiled durations
        # overlap with other contexts' launches there, so the throughput statement is work / (share x step time)
        dom_share = sum(ms for n, ms in rows if dominant(n) and (("+" in n) == fused)) / max(sum(ms for _, ms in rows), 1e-9)
        dom_work_step = (3.0 * flops if (fused and not args.half2 and not exact) else flops) * (tot_imgs / prof_runs)
        roofline = {"bound": bound, "kernel": kernel, "achieved": achieved, "peak": peak, "unit": unit, "frac": achieved / peak,
                    "frac_note": ("ALGORITHMIC work of the dominant launches (SURVEY.md 8d x images per launch%s) / their durations by HIP events on the launch "
                                  "stream in profiled steps of one context (%d stream(s)); %d launches x %.1f us %s one step of %.1f us: in the timed run the "
                                  "launches of %d contexts overlap -- frac_throughput / frac_step* are the throughput statements" % (
                                      "; x 3 fp16 MFMA products per multiply" if bound == "mfma" and not exact else "", spc, launches, avg_s * 1e6,
                                      ">" if overlapped else "<=", step_s * 1e6, nctx)),
                    "frac_executed": frac_executed,
                    "frac_throughput": dom_work_step / (dom_share * step_s) / (1e12 if bound == "mfma" else 1e9) / peak if bound == "mfma" else None,
                    "frac_throughput_note": "algorithmic work of one step's dominant launches / (their share of the profiled launch time x ms_per_step) / peak",
                    "dominant_share_of_launch_time": dom_share,
                    "overlapped": bool(overlapped), "traffic": traffic,
                    "traffic_unit": "bytes/launch (PMC pass %s)" % traffic_src,
                    "images_per_launch": avg_imgs,
                    "algorithmic_bytes": nbytes * avg_imgs, "flops_per_launch": flops * avg_imgs,
                    "avg_launch_us": avg_s * 1e6, "launches_per_step": launches,
                    "isolated_launch_us": iso_us, "isolated_images_per_launch": b_iso, "frac_isolated": iso_frac,
                    # whole step against the roofs: direct-form FLOPs of the network / fp32 matrix peak, and the minimum
                    # (perfectly fused) activation traffic of SURVEY.md 8d / HBM peak
                    "frac_step": NET_FLOPS * b / step_s / 1e12 / MFMA_F32_PEAK_TFLOPS,
                    "frac_step_note": "91.87 GFLOP (direct form) per pair / ms_per_step / 157.3 TFLOP/s fp32 matrix peak; above 1 is "
                                      "possible because the split kernels run on the fp16 pipe",
                    "frac_step_f16_split": 3.0 * NET_FLOPS * b / step_s / 1e12 / MFMA_F16_PEAK_TFLOPS,
                    "step_tflops": NET_FLOPS * b / step_s / 1e12,
                    # ... and the whole step against the HBM roof: algorithmic bytes of all launches layer by layer (each tensor once per
                    # launch that touches it; fp16 tensors in half2 mode) / step time -- what the overlapping contexts sustain
                    "step_algorithmic_bytes": net_bytes_2d() * (0.5 if args.half2 else 1.0) * b,
                    "step_gbs": net_bytes_2d() * (0.5 if args.half2 else 1.0) * b / step_s / 1e9,
                    "frac_step_hbm": net_bytes_2d() * (0.5 if args.half2 else 1.0) * b / step_s / 1e9 / HBM_PEAK_GBS,
                    # the same launch on round 1's scale (direct-form FLOPs / fp32 matrix peak, where the Winograd kernel had 0.63 / 0.69)
                    "direct_form_tflops": flops * tot_imgs / tot_s / 1e12, "direct_form_tflops_isolated": flops * b_iso / iso_us / 1e6,
                    "frac_of_fp32_mfma_peak": flops * tot_imgs / tot_s / 1e12 / MFMA_F32_PEAK_TFLOPS,
                    "frac_of_fp32_mfma_peak_isolated": flops * b_iso / iso_us / 1e6 / MFMA_F32_PEAK_TFLOPS,
                    "mfma_flops_executed": mfma_exec * avg_imgs,
                    "mfma_util_executed": mfma_exec * b_iso / iso_us / 1e6 / mfma_peak,
                    "mfma_util_note": "executed matrix FLOPs of one launch / isolated duration / %.0f TFLOP/s (%s pipe)" % (
                        mfma_peak, "fp32" if (exact and not args.half2) else "fp16"),
                    "hbm_gbs": nbytes * tot_imgs / tot_s / 1e9, "frac_hbm": nbytes * tot_imgs / tot_s / 1e9 / HBM_PEAK_GBS,
                    "frac_hbm_note": "algorithmic bytes of the same launches / in-situ duration / 8 TB/s"}
        if fused and not args.half2:
            roofline["bound_note"] = ("a 4-row step takes ~4.1 k cycles against 3.36 k for its MFMAs alone (two waves per SIMD share the "
                                      "matrix pipe; measured with the operand reads, the epilogue and the DMA switched off one by one, "
                                      "profiles/r06_rbs_dev.txt): within 20 % of the matrix pipe's floor for three fp16 products per multiply; the rest "
                                      "of `frac` is the 2.5 PFLOP/s peak assuming 2.4 GHz (sustained: 2.0-2.2), the 30-of-32 strip, the prologue and "
                                      "the pipeline's fill / drain steps (`frac_executed` counts those rows)")
        if fused and not args.half2:
            # continuity with the layer-by-layer kernel (the roofline object of earlier benches; still runs the other convolutions)
            g_us = isolated_dominant(lib.kernels, b, args.half2, fused=False)
            roofline["layer_by_layer_kernel"] = {"kernel": "conv_s3_kernel<3,3,1,il,il> 3x3 32->32 @629x185 (+bias,+residual,+ELU)", "bound": "hbm",
                                                 "isolated_launch_us": g_us, "algorithmic_bytes": DOMINANT_BYTES * b,
                                                 "achieved": DOMINANT_BYTES * b / g_us / 1e3, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                 "frac_isolated": DOMINANT_BYTES * b / g_us / 1e3 / HBM_PEAK_GBS}
    if rank == 0:
        out = {
            "metric": "stereo pairs/sec, ResNet18-2D 1257x369", "value": world * args.steps * b / elapsed,
            "unit": "pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "spinup": {"ms": args.spinup_ms, "untimed_steps": spun,
                       "why": "clock governor: the timed K steps follow W warm-up steps as contracted; before those the GPU is kept busy this long"},
            "ms_per_step": elapsed / args.steps * 1e3, "ms_per_pair": elapsed / args.steps / b * 1e3,
            "ms_per_pair_note": "1 / throughput with %d pairs in flight; latency_ms_per_pair (--full) is one pair through one context, synchronously" % nctx,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f16 (f32 accumulate)" if args.half2 else "f32", "data": "synthetic",
            "arithmetic": ("fp16 operands, fp32 accumulate (TensorRT half2 mode)" if args.half2 else
                           "fp32 fmaf chains on the fp32 matrix pipe (RT_CONV_EXACT_FP32=1)" if os.environ.get("RT_CONV_EXACT_FP32", "0") != "0" else
                           "fp32 tensors; convolutions as 3-term fp16 splits (22-bit operands, exact products) with fp32 accumulation "
                           "on the fp16 matrix pipe; correlation, soft-argmax, activations in fp32 -- error vs fp64 in the fp32-roundoff class"),
            "config": {"workload": "ResNet-18 2D Stereo DNN %s, 1257x369, batch=%d per step, one MI355X per rank" % (
                           "half2 mode" if args.half2 else "fp32", b),
                       "pairs_per_step": b, "contexts": nctx, "streams_per_context": spc, "launches_per_step": net.num_launches, "layers": net.num_layers,
                       "weights": weights_desc, "weights_transport": transport, "startup_degraded": bool(NATIVE_STARTUP_HUNG[0]), "parallelism": "pairs sharded over %d GPU(s)" % world},
            "ranks": rank_rows,
            "ranks_spread": {"pairs_per_s_min": min(r["pairs_per_s"] for r in rank_rows), "pairs_per_s_max": max(r["pairs_per_s"] for r in rank_rows),
                             "pairs_per_s_mean": sum(r["pairs_per_s"] for r in rank_rows) / len(rank_rows),
                             "host_issue_us_per_step_max": max(r["host_issue_us_per_step"] for r in rank_rows),
                             "note": "value = all ranks' pairs / the SLOWEST rank's time (max over ranks); host_issue_us_per_step is the host time one "
                                     "rank's thread spends issuing a step -- below step_us the host runs ahead of its GPU (profiles/r05_host_contention.txt: "
                                     "eight such processes side by side)"},
        }
        if args.full:
            out.update({
                "latency_ms_per_pair": single["synchronous_execute"]["ms_per_pair"] if single else None,
                "value_200": value_200, "value_exact_fp32": value_exact,
                "parity_max_abs_err": parity, "contexts_max_abs_diff": ctx_diff,
                "parity_note": "max |disp - oracle| over the %d timed context(s), same pair(s), %s; budget %s" % (
                    nctx, "oracle on the fp16-rounded weights" if args.half2 else "fp32 oracle", "1e-2" if args.half2 else "1e-3"),
                "roofline": roofline,
            })
        if single is not None:
            out["single_context"] = single
        if pcie is not None:
            out["pcie_inclusive"] = pcie
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(weights)
        if default_run:
            secondary = secondary_lines(lib, dev)
        if secondary is not None:
            out["secondary"] = secondary
        if last_disp is not None:
            dump_outputs(args.dump_outputs, {"disparity": last_disp})
        print(json.dumps(out), flush=True)
    for n in nets:
        n.destroy()
    if distributed:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
    if NATIVE_STARTUP_HUNG[0]:          # a thread is still inside the abandoned communicator bootstrap: do not wait for it at interpreter exit
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
