"""Camera frames in, disparity in pixels out: the ROS node's per-frame path (reference ros/packages/stereo_dnn_ros/src/
stereo_dnn_ros_node.cpp:42-103) on the device.

- rt_preprocess_frames_u8: both images of a pair batch, any of the RT_ENC_* encodings, pitched rows, one launch.  It must be
  bit-identical to rt_preprocess_bgr8 (pinned by the reference's img_left.bin in tests/test_imgproc_parity.py) on the dense BGR form of
  the same pixels.
- rt_disparity_scale: out = disp * scale, a single fp32 multiply.
- rt_net_execute_frames: pre-processing into net-owned inputs, the network, then RT_DISP_NET / RT_DISP_PIXELS_F32 / RT_DISP_KITTI_U16.
  Each kind must be bit-equal to the manual pipeline on the same engine (rt_preprocess_bgr8 x 2 -> execute -> x width for ResNet-18 2D,
  x 1 for the 3-D models, sample_app/main.cpp:325-327 -> 16-bit encoding).
CPU tier: the same sources on the SIMT emulator; GPU tier (-m gpu): the MI355X, the reference's sample pair and trained weights."""
import os

import numpy as np
import pytest
import torch

from oracle import stereo_oracle as O
from redtail_amd import build, capi, model_files

ENCODINGS = [capi.RT_ENC_BGR8, capi.RT_ENC_RGB8, capi.RT_ENC_BGRA8, capi.RT_ENC_RGBA8]
PAD = 13                  # bytes of padding behind every row of a pitched frame (not a multiple of 4: no dword alignment)
PAD_BYTE = 0xAB


def pack(bgr, encoding, pad=0, seed=0):
    """(N,H,W,3) BGR uint8 -> (N,H,step) frames in `encoding`, step = W * bytes per pixel + pad, padding bytes PAD_BYTE"""
    n, h, w, _ = bgr.shape
    px = bgr if encoding in (capi.RT_ENC_BGR8, capi.RT_ENC_BGRA8) else bgr[..., ::-1]
    if capi.ENC_BYTES[encoding] == 4:        # alpha: random, it must be dropped
        alpha = np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 1), dtype=np.uint8)
        px = np.concatenate([px, alpha], axis=3)
    rows = px.reshape(n, h, -1)
    out = np.full((n, h, rows.shape[2] + pad), PAD_BYTE, np.uint8)
    out[:, :, :rows.shape[2]] = rows
    return out


def images(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


class Dev:
    """buffers on the backend: numpy under the emulator, torch device tensors on the GPU"""

    def __init__(self, gpu):
        self.gpu = gpu

    def put(self, a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a).cuda() if self.gpu else a.copy()

    def nan(self, *shape):
        return torch.full(shape, float("nan"), device="cuda") if self.gpu else np.full(shape, np.nan, np.float32)

    def u16(self, *shape):
        return torch.zeros(shape, dtype=torch.int16, device="cuda") if self.gpu else np.zeros(shape, np.uint16)

    def get(self, t):
        if not self.gpu:
            return np.array(t)
        torch.cuda.synchronize()
        a = t.cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a


# ---- rt_preprocess_frames_u8 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, PAD], ids=["dense", "pitched"])
@pytest.mark.parametrize("encoding", ENCODINGS, ids=["bgr8", "rgb8", "bgra8", "rgba8"])
@pytest.mark.parametrize("src,dst", [((37, 59), (37, 59)), ((375, 1242), (321, 1025)), ((40, 66), (20, 33)), ((50, 97), (9, 17))])
def test_preprocess_frames_bit_equal_to_preprocess_bgr8(backend, src, dst, encoding, pad):
    d = Dev(backend.name == "gpu")
    n = 2
    left, right = images(n, *src, seed=3), images(n, *src, seed=4)           # different contents: a swapped pair fails
    fl, fr = pack(left, encoding, pad, 1), pack(right, encoding, pad, 2)
    step = fl.shape[2]
    ol, orr = d.nan(n, 3, *dst), d.nan(n, 3, *dst)
    backend.klib.preprocess_frames_u8(d.put(fl), d.put(fr), src[0], src[1], step, encoding, ol, orr, dst[0], dst[1], n)
    got_l, got_r = d.get(ol), d.get(orr)
    for img, got in ((left, got_l), (right, got_r)):
        ref = d.nan(n, 3, *dst)
        backend.klib.preprocess_bgr8(d.put(img), src[0], src[1], ref, dst[0], dst[1], n)
        assert np.array_equal(got, d.get(ref))                               # bit-equal, NaN-free (array_equal fails on NaN)
        oracle = np.stack([O.preprocess_bgr8(img[i], *dst) for i in range(n)])
        assert np.abs(got - oracle).max() <= 2e-6


def test_preprocess_frames_refusals(backend):
    """up-scaling, factors above 6, a short step, an unknown encoding, null pointers: RtError, and nothing is written"""
    d = Dev(backend.name == "gpu")
    k = backend.klib
    img = pack(images(1, 70, 70, 5), capi.RT_ENC_BGRA8)
    src = d.put(img)
    ol, orr = d.nan(1, 3, 80, 80), d.nan(1, 3, 80, 80)
    cases = [
        (src, src, 70, 70, 280, capi.RT_ENC_BGRA8, ol, orr, 80, 80),        # up-scaling
        (src, src, 70, 70, 280, capi.RT_ENC_BGRA8, ol, orr, 70, 80),        # up-scaling along one axis
        (src, src, 70, 70, 280, capi.RT_ENC_BGRA8, ol, orr, 10, 10),        # factor 7
        (src, src, 70, 70, 279, capi.RT_ENC_BGRA8, ol, orr, 35, 35),        # step shorter than 70 pixels of 4 bytes
        (src, src, 70, 70, 209, capi.RT_ENC_BGR8, ol, orr, 35, 35),         # ... of 3 bytes
        (src, src, 70, 70, 280, 4, ol, orr, 35, 35),                        # unknown encodings
        (src, src, 70, 70, 280, -1, ol, orr, 35, 35),
        (None, src, 70, 70, 280, capi.RT_ENC_BGRA8, ol, orr, 35, 35),       # null pointers
        (src, None, 70, 70, 280, capi.RT_ENC_BGRA8, ol, orr, 35, 35),
        (src, src, 70, 70, 280, capi.RT_ENC_BGRA8, None, orr, 35, 35),
        (src, src, 70, 70, 280, capi.RT_ENC_BGRA8, ol, None, 35, 35),
    ]
    for i, args in enumerate(cases):
        with pytest.raises(capi.RtError):
            k.preprocess_frames_u8(*args, 1)
        assert np.isnan(d.get(ol)).all() and np.isnan(d.get(orr)).all(), i
    k.preprocess_frames_u8(src, src, 70, 70, 280, capi.RT_ENC_BGRA8, ol, orr, 35, 35, 1)    # and the valid call next to them works
    assert not np.isnan(d.get(ol).reshape(-1)[:3 * 35 * 35]).any()


def test_disparity_scale(backend):
    d = Dev(backend.name == "gpu")
    rng = np.random.default_rng(9)
    x = np.concatenate([np.float32([0.0, -0.0, 1.0, 1e-30, 3e30, -2.5]), rng.uniform(0, 1, 4097).astype(np.float32)])
    for scale in (513.0, 1.0, 1.0 / 3.0, 1257.0):
        ref = x * np.float32(scale)
        src, out = d.put(x), d.nan(x.size)
        backend.klib.disparity_scale(src, out, x.size, scale)
        assert np.array_equal(d.get(out), ref), scale
        backend.klib.disparity_scale(src, src, x.size, scale)                 # in place
        assert np.array_equal(d.get(src), ref), scale
    with pytest.raises(capi.RtError):
        backend.klib.disparity_scale(None, d.nan(4), 4, 2.0)


# ---- rt_net_execute_frames on synthetic weights -------------------------------------------------------------------------------------------
_nets = {}


def netlib(kind):
    if kind not in _nets:
        _nets[kind] = capi.NetLib(build.build_host_emu(), build.build_emu()) if kind == "emu" else capi.NetLib()
    return _nets[kind]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def rt(request):
    return request.param


def manual(lib, d, net, left_bgr, right_bgr, h, w):
    """the 4-launch pipeline a caller writes today: rt_preprocess_bgr8 x 2 -> rt_net_execute (the net's raw output)"""
    n, sh, sw, _ = left_bgr.shape
    il, ir, out = d.nan(n, 3, h, w), d.nan(n, 3, h, w), d.nan(n, 1, h, w)
    lib.kernels.preprocess_bgr8(d.put(left_bgr), sh, sw, il, h, w, n)
    lib.kernels.preprocess_bgr8(d.put(right_bgr), sh, sw, ir, h, w, n)
    net.execute(il, ir, out, n)
    return d.get(out)


def check_kinds(lib, d, net, left_bgr, right_bgr, h, w, scale, encoding=capi.RT_ENC_BGRA8, pad=PAD, stream=None):
    n = left_bgr.shape[0]
    raw = manual(lib, d, net, left_bgr, right_bgr, h, w)
    assert not np.isnan(raw).any()
    fl, fr = d.put(pack(left_bgr, encoding, pad, 11)), d.put(pack(right_bgr, encoding, pad, 12))
    sw = left_bgr.shape[2]
    got = {}
    for kind in (capi.RT_DISP_NET, capi.RT_DISP_PIXELS_F32, capi.RT_DISP_KITTI_U16):
        out = d.u16(n, 1, h, w) if kind == capi.RT_DISP_KITTI_U16 else d.nan(n, 1, h, w)
        net.execute_frames(fl, fr, encoding, out, kind=kind, batch=n, stream=stream, src_w=sw)
        got[kind] = d.get(out)
    pixels = raw * np.float32(scale)
    assert np.array_equal(got[capi.RT_DISP_NET], raw)
    assert np.array_equal(got[capi.RT_DISP_PIXELS_F32], pixels)
    assert np.array_equal(got[capi.RT_DISP_KITTI_U16], O.disparity_to_u16(raw, 256.0 * scale))
    assert np.array_equal(got[capi.RT_DISP_KITTI_U16], O.disparity_to_u16(pixels, 256.0))     # main.cpp: *= 256, then *= w
    return raw, got


@pytest.mark.parametrize("model,flags", [("resnet18_2D", 0), ("resnet18_2D", capi.RT_CONV_EXACT_FP32), ("nvtiny", 0)],
                         ids=["resnet18_2D", "resnet18_2D-exact", "nvtiny"])
def test_execute_frames_equals_manual_pipeline(rt, model, flags):
    """bgra8 frames with a padded step from an 83x51 source, batch 2 = max_batch; all three kinds bit-equal to the manual pipeline"""
    lib, d = netlib(rt), Dev(rt == "gpu")
    if model == "resnet18_2D":
        h, w, weights, disp = 25, 41, O.synth_weights_resnet18_2d(), 8
    else:
        h, w, weights, disp = 25, 33, O.synth_weights_3d(O.NVTINY_3D), 4
    net = lib.create(model, w, h, max_batch=2, weights=weights, max_disp=disp, flags=flags)
    left, right = images(2, 51, 83, 21), images(2, 51, 83, 22)
    check_kinds(lib, d, net, left, right, h, w, scale=w if model == "resnet18_2D" else 1)
    # the frame tensor forms the binding accepts: (N,H,W,C) dense, and (N,H,W,C) views of padded rows
    ref = d.nan(2, 1, h, w)
    net.execute_frames(d.put(pack(left, capi.RT_ENC_RGB8)), d.put(pack(right, capi.RT_ENC_RGB8)), capi.RT_ENC_RGB8, ref,
                       kind=capi.RT_DISP_NET, batch=2, src_w=83)
    ref = d.get(ref)
    dense = [d.put(pack(img, capi.RT_ENC_RGBA8).reshape(2, 51, 83, 4)) for img in (left, right)]
    padded = [d.put(pack(img, capi.RT_ENC_RGBA8, PAD + 3)) for img in (left, right)]              # rows of 348 bytes
    shape, strides = (2, 51, 83, 4), (51 * 348, 348, 4, 1)
    views = [p.as_strided(shape, strides) if d.gpu else np.lib.stride_tricks.as_strided(p, shape, strides) for p in padded]
    for fl, fr in (dense, views):
        out = d.nan(2, 1, h, w)
        net.execute_frames(fl, fr, capi.RT_ENC_RGBA8, out, kind=capi.RT_DISP_NET, batch=2)
        assert np.array_equal(d.get(out), ref)
    # batch > max_batch, unknown kind or encoding, up-scaling: RtError and nothing written
    out = d.nan(3, 1, h, w)
    f3l, f3r = d.put(pack(images(3, 51, 83, 1), capi.RT_ENC_BGR8)), d.put(pack(images(3, 51, 83, 2), capi.RT_ENC_BGR8))
    small = d.put(pack(images(2, 20, 30, 1), capi.RT_ENC_BGR8))
    for args, kw in (((f3l, f3r, capi.RT_ENC_BGR8, out), dict(batch=3, src_w=83)),
                     ((f3l, f3r, capi.RT_ENC_BGR8, out), dict(batch=2, src_w=83, kind=3)),
                     ((f3l, f3r, capi.RT_ENC_BGR8, out), dict(batch=2, src_w=83, kind=-1)),
                     ((f3l, f3r, 7, out), dict(batch=2, src_w=83)),
                     ((small, small, capi.RT_ENC_BGR8, out), dict(batch=2, src_w=30))):
        with pytest.raises(capi.RtError):
            net.execute_frames(*args, **kw)
        assert np.isnan(d.get(out)).all()
    net.destroy()


def test_execute_frames_on_a_plan_built_net(rt):
    """rt_net_create_from_plan recovers the input size and the model (ResNet-18 2D: x width) from the plan"""
    lib, d = netlib(rt), Dev(rt == "gpu")
    net = lib.create("resnet18_2D", 41, 25, max_batch=2, weights=O.synth_weights_resnet18_2d(), max_disp=8)
    left, right = images(2, 51, 83, 31), images(2, 51, 83, 32)
    _, ref = check_kinds(lib, d, net, left, right, 25, 41, scale=41)
    net2 = lib.create_from_plan(net.serialize(), 0, 0)          # the Python-side size is not used by the C entry
    net.destroy()
    _, got = check_kinds(lib, d, net2, left, right, 25, 41, scale=41)
    for kind in ref:
        assert np.array_equal(got[kind], ref[kind]), kind
    net2.destroy()


# ---- GPU only: the reference's sample pair and trained weights, graph mode and streams ---------------------------------------------------
def sample_bgr():
    from PIL import Image
    return [np.ascontiguousarray(np.array(Image.open(model_files.sample_image(side)).convert("RGB"))[None, :, :, ::-1])
            for side in ("left", "right")]


@pytest.mark.gpu
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16-half2"])
def test_reference_sample_pair_resnet18_2d(fp16):
    lib, d = netlib("gpu"), Dev(True)
    w, h = 513, 257
    net = lib.create("resnet18_2D", w, h, weights_path=model_files.weight_file("resnet18_2D", fp16), fp16_weights=fp16)
    left, right = sample_bgr()
    raw, got = check_kinds(lib, d, net, left, right, h, w, scale=w)
    net.destroy()
    if not fp16:
        l, r = (O.preprocess_bgr8(img[0], h, w) for img in (left, right))
        with torch.no_grad():
            ref = O.resnet18_2d(torch.from_numpy(l)[None], torch.from_numpy(r)[None],
                                O.read_weights(model_files.weight_file("resnet18_2D"))).numpy()
        err = np.abs(got[capi.RT_DISP_PIXELS_F32] - ref * w).max()
        print("execute_frames resnet18_2D 513x257 fp32 on the sample pair: max |px - oracle px| = %.3g" % err)
        assert err <= 1e-3 * w, err


@pytest.mark.gpu
def test_reference_sample_pair_nvtiny():
    lib, d = netlib("gpu"), Dev(True)
    net = lib.create("nvtiny", 513, 161, weights_path=model_files.weight_file("nvtiny"))
    left, right = sample_bgr()
    raw, got = check_kinds(lib, d, net, left, right, 161, 513, scale=1)
    assert np.array_equal(got[capi.RT_DISP_PIXELS_F32], raw)          # already in pixels: x 1
    net.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("streams", [2, 1])
def test_graph_mode_with_rotating_buffers(streams):
    """a camera ring buffer: three sets of frame and output buffers in rotation, on a torch stream and on the NULL stream, with graph
    mode on -- every result bit-equal to the direct path"""
    lib, d = netlib("gpu"), Dev(True)
    h, w, n = 129, 257, 2
    net = lib.create("resnet18_2D", w, h, max_batch=n, weights=O.synth_weights_resnet18_2d(), max_disp=16)
    net.set_streams(streams)
    sets = []
    for i in range(3):
        left, right = images(n, 376, 672, 40 + 2 * i), images(n, 376, 672, 41 + 2 * i)
        sets.append((d.put(pack(left, capi.RT_ENC_BGRA8, PAD, i)), d.put(pack(right, capi.RT_ENC_BGRA8, PAD, i + 7))))
    src_w = 672

    def run(i, out, stream=None):
        net.execute_frames(sets[i][0], sets[i][1], capi.RT_ENC_BGRA8, out, kind=capi.RT_DISP_PIXELS_F32, batch=n, stream=stream,
                           src_w=src_w)

    direct = []
    for i in range(3):
        out = d.nan(n, 1, h, w)
        run(i, out)
        direct.append(d.get(out))
    assert not np.isnan(direct[0]).any() and not np.array_equal(direct[0], direct[1])
    net.set_graph(True)
    outs = [d.nan(n, 1, h, w) for _ in range(3)]
    s = torch.cuda.Stream()
    for call in range(9):                                 # 1: direct, 2: capture + launch, then replays, whatever pointers rotate in
        i = call % 3
        outs[i].fill_(float("nan"))
        torch.cuda.synchronize()
        run(i, outs[i], stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(d.get(outs[i]), direct[i]), call
    for call in range(6):
        i = (call + 1) % 3
        outs[i].fill_(float("nan"))
        torch.cuda.synchronize()
        run(i, outs[i])
        assert np.array_equal(d.get(outs[i]), direct[i]), call
    net.destroy()


@pytest.mark.gpu
def test_plan_built_net_trained_weights():
    """create_from_plan(net.serialize()) + execute_frames == the original net on the reference's sample pair"""
    lib, d = netlib("gpu"), Dev(True)
    net = lib.create("resnet18_2D", 513, 257, weights_path=model_files.weight_file("resnet18_2D"))
    left, right = sample_bgr()
    _, ref = check_kinds(lib, d, net, left, right, 257, 513, scale=513)
    net2 = lib.create_from_plan(net.serialize(), 513, 257)
    net.destroy()
    _, got = check_kinds(lib, d, net2, left, right, 257, 513, scale=513)
    for kind in ref:
        assert np.array_equal(got[kind], ref[kind]), kind
    net2.destroy()
