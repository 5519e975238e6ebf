"""The viz node's 2x2 debug panel (reference ros/packages/stereo_dnn_ros_viz/src/stereo_dnn_ros_viz_node.cpp) on the device, rgb8:

    left frame, area-resized  | right frame, area-resized
    disparity as grey         | disparity in the KITTI colour scheme

- rt_disparity_to_color: the colour picture alone; rt_viz_mosaic_u8: the whole panel in one launch.  The two disparity panels are defined
  operation by operation (include/rt_stereo.h), so `color_ref` / `grey_ref` below (numpy float32 / float64) are bit-exact: no tolerance.
- The frame panels are rint (ties to even) of the fp32 area average of rt_preprocess_frames_u8: exact where the average is exact, and
  equal to the rounded CPU oracle everywhere but within 2e-3 of a rounding tie, where either neighbour is accepted.
- rt_net_execute_frames_viz: rt_net_execute_frames / rt_net_execute_frames_lr followed by the panel of the disparity just written.
CPU tier: the same sources on the SIMT emulator; GPU tier (-m gpu): the MI355X, plus the reference's sample pair with trained weights."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import stereo_oracle as O
from redtail_amd import capi, model_files
from test_camera_frames import ENCODINGS, PAD, Dev, images, netlib, pack, rt, sample_bgr  # noqa: F401  (rt: the emu / gpu fixture)
from test_lr_consistency import Bufs, call_lr, make_net

FILL = 0xCD               # every output byte before a call: a byte left unwritten, or written where it should not be, shows
WEIGHTS = np.float32([8.77192974, 5.40540552, 8.77192974, 5.74712658, 8.77192974, 5.40540552, 8.77192974, 0])
CUMSUM = np.float32([0, 0.114, 0.299, 0.413, 0.587, 0.70100003, 0.88600004, 1])
W_MAP = np.array([[i >> 1 & 1, i >> 2 & 1, i & 1] for i in range(8)] + [[0, 0, 0]])       # row 8: what the reference reads past its table


# ---- the two disparity panels restated in numpy --------------------------------------------------------------------------------------------
def color_ref(d, max_disp):
    """(..., 3) uint8 R,G,B of the KITTI colour scheme as include/rt_stereo.h defines it"""
    d = np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        cur = d / np.float32(max_disp)
        index = np.zeros(d.shape, np.int64)
        for i in range(1, 8):
            index = np.where(cur > CUMSUM[i], i, index)                                  # cumsum rises: the last hit is the largest
        x = (cur - CUMSUM[index]) * WEIGHTS[index]                                       # float32, each operation rounded on its own
        assert x.dtype == np.float32
        w = (1.0 - x.astype(np.float64)).astype(np.float32).astype(np.float64)
        w = np.where(index == 7, 1.0, w)                                                 # weight 0: w = 1 by definition, also for inf
        u = 1.0 - w
        v = (np.where(W_MAP[index] == 1, w[..., None], 0.0) + np.where(W_MAP[index + 1] == 1, u[..., None], 0.0)) * 255.0
        v = np.where(v > 0, np.minimum(v, 255.0), 0.0)                                   # NaN and negative: 0
    return np.trunc(v).astype(np.uint8)


def grey_ref(d, max_disp):
    d = np.asarray(d, np.float32)
    s = np.float32(255) / np.float32(max_disp)
    with np.errstate(all="ignore"):
        v = np.rint(d * s)
        assert v.dtype == np.float32
        v = np.where(v > 0, np.minimum(v, np.float32(255)), np.float32(0))
    return np.repeat(v.astype(np.uint8)[..., None], 3, axis=-1)


def disparity_cases(max_disp, count, seed):
    """the table's own values and their fp32 neighbours, the special values, then uniform ones in [-5, 1.2 max_disp]"""
    m = np.float32(max_disp)
    edges = np.concatenate([[c, np.nextafter(c, np.float32(-1)), np.nextafter(c, np.float32(2))] for c in CUMSUM]).astype(np.float32) * m
    special = np.float32([0.0, -0.0, -3.25, max_disp, 1.5 * max_disp, 1e30, np.nan, np.inf, -np.inf, -1e38, 1e-30])
    rnd = np.random.default_rng(seed).uniform(-5.0, 1.2 * max_disp, count).astype(np.float32)
    out = np.concatenate([edges, special, rnd])[:count]
    assert out.size == count and count >= edges.size + special.size + 3000
    return out


def test_restatement_anchors():
    """hand-checked values of the restatement itself"""
    for m in (96.0, 68.0):
        assert color_ref(np.float32([0.0, -0.0]), m).tolist() == [[0, 0, 0], [0, 0, 0]] and grey_ref(np.float32([0.0]), m).tolist() == [[0, 0, 0]]
        big = np.float32([1.01 * m, 1.5 * m, 1e30, np.inf])
        assert (color_ref(big, m) == 255).all() and (grey_ref(big, m) == 255).all()
        bad = np.float32([np.nan, -1.0, -np.inf, -1e38])
        assert (color_ref(bad, m) == 0).all() and (grey_ref(bad, m) == 0).all()
    # the corner colours: at cumsum[i] * max_disp + a little, the colour is w_map[i] (blue, red, magenta, green, cyan, yellow)
    assert color_ref(np.float32([0.114 * 96 + 1e-3]), 96.0).tolist() == [[0, 0, 254]]
    assert color_ref(np.float32([0.299 * 96 + 1e-3]), 96.0).tolist() == [[255, 0, 0]]       # red in both corners: w + (1 - w) = 1 exactly
    assert color_ref(np.float32([0.587 * 96 + 1e-3]), 96.0).tolist() == [[0, 255, 0]]
    assert color_ref(np.float32([0.5 * (0.114 + 0.299) * 96]), 96.0).tolist() == [[127, 0, 127]]      # half way from blue to red: 127.5 truncated
    top = color_ref(np.float32([96.0]), 96.0)[0]             # cur = 1 is not > 1: the end of the yellow-to-white segment
    assert top[0] == 255 and top[1] == 255 and top[2] >= 254
    assert grey_ref(np.float32([48.0, 0.5 * 96 / 255, 1.5 * 96 / 255]), 96.0)[:, 0].tolist() == [128, 0, 2]       # 127.5 -> 128, ties to even


def out_buf(d, n, rows, step):
    return d.put(np.full((n, rows, step), FILL, np.uint8))


def panels(buf, h, w):
    """(n, 2h, step) bytes -> the four (n,h,w,3) panels and the padding"""
    n = buf.shape[0]
    px = buf[:, :, :6 * w].reshape(n, 2 * h, 2 * w, 3)
    return dict(tl=px[:, :h, :w], tr=px[:, :h, w:], bl=px[:, h:, :w], br=px[:, h:, w:], pad=buf[:, :, 6 * w:])


# ---- 1. colour and grey panels, bit-exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_disp", [96.0, 68.0])
@pytest.mark.parametrize("h,w", [(130, 17), (5, 513), (3, 1257)])
def test_disparity_panels_bit_exact(backend, h, w, max_disp):
    d = Dev(backend.name == "gpu")
    k = backend.klib
    n = 2
    disp = disparity_cases(max_disp, n * h * w, seed=w).reshape(n, 1, h, w)
    dd = d.put(disp)
    color, grey = color_ref(disp[:, 0], max_disp), grey_ref(disp[:, 0], max_disp)
    flat, cflat = disp.reshape(-1), color.reshape(-1, 3)
    nan = np.isnan(flat)
    assert (cflat[flat == 0] == 0).all() and (cflat[flat > np.float32(max_disp)] == 255).all() and (cflat[nan] == 0).all()
    assert (grey.reshape(-1, 3)[nan] == 0).all() and (flat == 0).sum() >= 2 and nan.any() and (flat > np.float32(max_disp)).sum() > 100
    for pad in (0, 10):                                  # 3 w + 10 is 1 modulo 4 for all three widths: rows start at every alignment
        step = 3 * w + pad
        assert pad == 0 or step % 4 == 1
        out = out_buf(d, n, h, step)
        k.disparity_to_color(dd, n, h, w, max_disp, out, step)
        got = d.get(out)
        assert np.array_equal(got[:, :, :3 * w].reshape(n, h, w, 3), color), pad
        assert (got[:, :, 3 * w:] == FILL).all()
    frames = images(n, h, w, 7)                          # same size: the top panels are the frames
    f = d.put(pack(frames, capi.RT_ENC_BGR8))
    for pad in (0, PAD):                                 # 6 w + 13 is 3 modulo 4
        step = 6 * w + pad
        out = out_buf(d, n, 2 * h, step)
        k.viz_mosaic_u8(f, f, h, w, 3 * w, capi.RT_ENC_BGR8, dd, h, w, max_disp, out, step, n)
        got = panels(d.get(out), h, w)
        assert np.array_equal(got["br"], color) and np.array_equal(got["bl"], grey), pad
        assert np.array_equal(got["tl"], frames[..., ::-1]) and np.array_equal(got["tr"], frames[..., ::-1]), pad
        assert (got["pad"] == FILL).all()


# ---- 2. rt_disparity_to_color is the bottom-right panel --------------------------------------------------------------------------------------------
def test_disparity_to_color_equals_the_mosaic_panel(backend):
    d = Dev(backend.name == "gpu")
    k = backend.klib
    n, h, w, sh, sw = 2, 21, 67, 50, 97
    disp = d.put(np.random.default_rng(1).uniform(-2, 110, (n, 1, h, w)).astype(np.float32))
    left, right = d.put(pack(images(n, sh, sw, 1), capi.RT_ENC_RGBA8, PAD)), d.put(pack(images(n, sh, sw, 2), capi.RT_ENC_RGBA8, PAD))
    mosaic, color = out_buf(d, n, 2 * h, 6 * w + 3), out_buf(d, n, h, 3 * w)
    k.viz_mosaic_u8(left, right, sh, sw, 4 * sw + PAD, capi.RT_ENC_RGBA8, disp, h, w, 96.0, mosaic, 6 * w + 3, n)
    k.disparity_to_color(disp, n, h, w, 96.0, color)
    assert np.array_equal(panels(d.get(mosaic), h, w)["br"], d.get(color).reshape(n, h, w, 3))
    assert len(np.unique(d.get(color))) > 100


# ---- 3. frame panels ----------------------------------------------------------------------------------------------------------------------------
def frame_panel_ok(got, bgr, dst):
    """got: (n,h,w,3) R,G,B panel of the (n,sh,sw,3) BGR frames.  Returns the share of near-tie values (a condition on the oracle alone)"""
    n, sh, sw, _ = bgr.shape
    h, w = dst
    if (sh, sw) == (h, w):
        assert np.array_equal(got, bgr[..., ::-1])
        return 0.0
    if (sh, sw) == (2 * h, 2 * w):                      # every sum is exact in fp32; a quarter of the values are exact ties
        mean = bgr.astype(np.float64).reshape(n, h, 2, w, 2, 3).mean(axis=(2, 4))
        assert (mean - np.floor(mean) == 0.5).mean() > 0.2
        assert np.array_equal(got, np.rint(mean).astype(np.uint8)[..., ::-1])
        return 0.0
    v = 255.0 * np.stack([O.preprocess_bgr8(bgr[i], h, w) for i in range(n)]).astype(np.float64).transpose(0, 2, 3, 1)   # (n,h,w,RGB)
    near = np.abs((v - np.floor(v)) - 0.5) < 2e-3
    ok = (got == np.rint(v)) | (near & ((got == np.floor(v)) | (got == np.ceil(v))))
    assert ok.all(), int((~ok).sum())
    return float(near.mean())


@pytest.mark.parametrize("pad", [0, PAD], ids=["dense", "pitched"])
@pytest.mark.parametrize("encoding", ENCODINGS, ids=["bgr8", "rgb8", "bgra8", "rgba8"])
@pytest.mark.parametrize("src,dst", [((37, 59), (37, 59)), ((375, 1242), (321, 1025)), ((40, 66), (20, 33)), ((50, 97), (9, 17))])
def test_frame_panels(backend, src, dst, encoding, pad):
    d = Dev(backend.name == "gpu")
    n = 2
    h, w = dst
    left, right = images(n, *src, seed=3), images(n, *src, seed=4)           # different contents: a swapped pair fails
    fl, fr = pack(left, encoding, pad, 1), pack(right, encoding, pad, 2)
    disp = np.random.default_rng(5).uniform(0, 96, (n, 1, h, w)).astype(np.float32)
    step = 6 * w + pad
    out = out_buf(d, n, 2 * h, step)
    backend.klib.viz_mosaic_u8(d.put(fl), d.put(fr), src[0], src[1], fl.shape[2], encoding, d.put(disp), h, w, 96.0, out, step, n)
    got = panels(d.get(out), h, w)
    assert not np.array_equal(got["tl"], got["tr"])
    for name, img in (("tl", left), ("tr", right)):                         # top-left is left
        share = frame_panel_ok(got[name], img, dst)
        assert share < 0.02, share
    assert np.array_equal(got["br"], color_ref(disp[:, 0], 96.0)) and np.array_equal(got["bl"], grey_ref(disp[:, 0], 96.0))
    assert (got["pad"] == FILL).all()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(backend):
    """up-scaling, a factor above 6, short steps, an unknown encoding, null pointers, batch < 1, a max_disp that is no number > 0: RtError,
    and every output byte keeps its value; then the valid call next to them works"""
    d = Dev(backend.name == "gpu")
    k = backend.klib
    src = d.put(pack(images(1, 70, 70, 5), capi.RT_ENC_BGRA8))
    disp = d.put(np.full((1, 1, 80, 80), 40.0, np.float32))
    out = out_buf(d, 1, 160, 480)
    E = capi.RT_ENC_BGRA8
    ok = dict(left=src, right=src, src_h=70, src_w=70, src_step=280, encoding=E, disp_px=disp, h=35, w=35, max_disp=96.0, dst_rgb8=out,
              dst_step=210, batch=1)
    cases = [dict(h=80, w=80, dst_step=480), dict(h=70, w=80, dst_step=480), dict(h=80, w=70, dst_step=420),      # up-scaling
             dict(h=10, w=10, dst_step=60),                                                                       # factor 7
             dict(src_step=279), dict(src_step=209, encoding=capi.RT_ENC_BGR8),                                   # short source rows
             dict(dst_step=209), dict(dst_step=0), dict(dst_step=-210),                                           # short panel rows
             dict(encoding=4), dict(encoding=-1),
             dict(left=None), dict(right=None), dict(disp_px=None), dict(dst_rgb8=None),
             dict(batch=0), dict(batch=-1),
             dict(max_disp=0.0), dict(max_disp=-96.0), dict(max_disp=float("nan")), dict(max_disp=float("inf"))]
    for i, change in enumerate(cases):
        with pytest.raises(capi.RtError):
            k.viz_mosaic_u8(**dict(ok, **change))
        assert (d.get(out) == FILL).all(), i
    okc = dict(disp_px=disp, batch=1, h=35, w=35, max_disp=96.0, dst_rgb8=out, dst_step=105)
    for i, change in enumerate([dict(dst_step=104), dict(disp_px=None), dict(dst_rgb8=None), dict(batch=0), dict(max_disp=0.0),
                                dict(max_disp=float("nan")), dict(h=0), dict(w=0)]):
        with pytest.raises(capi.RtError):
            k.disparity_to_color(**dict(okc, **change))
        assert (d.get(out) == FILL).all(), i
    k.viz_mosaic_u8(**ok)
    got = d.get(out).reshape(-1)
    assert (got[70 * 210:] == FILL).all() and (got[:70 * 210] != FILL).mean() > 0.9
    out2 = out_buf(d, 1, 35, 105)
    k.disparity_to_color(**dict(okc, dst_rgb8=out2))
    assert np.array_equal(d.get(out2).reshape(35, 35, 3), color_ref(np.full((35, 35), 40.0, np.float32), 96.0))


# ---- 5. rt_net_execute_frames_viz on synthetic weights ------------------------------------------------------------------------------------------
MAX_DISP = 24.0           # the synthetic nets' disparities span a few tens of pixels: most of the colour range is used


def make_stream(lib, gpu):
    if gpu:
        s = torch.cuda.Stream()
        return s.cuda_stream, s.synchronize, lambda: None, s
    handle = ctypes.c_void_p()
    lib.kernels.check(lib.kernels.lib.rt_stream_create(ctypes.byref(handle)), "rt_stream_create")
    stream = handle.value
    return (stream, lambda: lib.kernels.check(lib.kernels.lib.rt_stream_sync(stream), "rt_stream_sync"),
            lambda: lib.kernels.lib.rt_stream_destroy(stream), None)


@pytest.mark.parametrize("model", ["resnet18_2D", "nvtiny"])
def test_execute_frames_viz_equals_the_calls_it_wraps(rt, model):
    lib, d = netlib(rt), Bufs(rt == "gpu")
    net, h, w, _ = make_net(lib, model)                              # max_batch 4
    enc, sh, sw = capi.RT_ENC_BGRA8, 51, 83
    stream, sync, destroy, keep = make_stream(lib, rt == "gpu")
    kind = capi.RT_DISP_PIXELS_F32
    for n in (1, 2):
        left, right = images(n, sh, sw, 21 + n), images(n, sh, sw, 31 + n)
        fl, fr = d.put(pack(left, enc, PAD, 11)), d.put(pack(right, enc, PAD, 12))
        sstep = fl.shape[2]
        ref = d.nan(n, 1, h, w)
        net.execute_frames(fl, fr, enc, ref, kind=kind, batch=n, src_w=sw)
        ref = d.get(ref)
        assert not np.isnan(ref).any()
        ref_lr = d.read(call_lr(d, net, fl, fr, enc, n, h, w, kind, 1.0, src_w=sw), kind)
        assert 0 < ref_lr["valid_count"].sum() < n * h * w
        for s, vsteps in ((None, (6 * w,)), (stream, (6 * w + PAD,) if rt != "gpu" else (6 * w, 6 * w + PAD))):
            for vstep in vsteps:
                # no check
                disp, viz = d.nan(n, 1, h, w), out_buf(d, n, 2 * h, vstep)
                net.execute_frames_viz(fl, fr, enc, disp, viz, viz_step=vstep, max_disp=MAX_DISP, batch=n, stream=s, src_w=sw)
                if s is not None:
                    sync()
                assert np.array_equal(d.get(disp), ref)
                want = out_buf(d, n, 2 * h, vstep)
                lib.kernels.viz_mosaic_u8(fl, fr, sh, sw, sstep, enc, disp, h, w, MAX_DISP, want, vstep, n)
                got = d.get(viz)
                assert np.array_equal(got, d.get(want))
                p = panels(got, h, w)
                assert np.array_equal(p["br"], color_ref(ref[:, 0], MAX_DISP)) and np.array_equal(p["bl"], grey_ref(ref[:, 0], MAX_DISP))
                assert (p["pad"] == FILL).all() and len(np.unique(p["br"])) > 20
                # with the left-right check
                bufs, viz = d.outputs(n, h, w, kind), out_buf(d, n, 2 * h, vstep)
                net.execute_frames_viz(fl, fr, enc, bufs["out"], viz, viz_step=vstep, max_disp=MAX_DISP, max_diff_px=1.0, mask=bufs["mask"],
                                       valid_count=bufs["valid_count"], batch=n, stream=s, src_w=sw)
                if s is not None:
                    sync()
                got_lr = d.read(bufs, kind)
                for key in ("out", "mask", "valid_count"):
                    assert np.array_equal(got_lr[key], ref_lr[key]), key
                assert np.isnan(got_lr["right_out"]).all()           # not an output of this call
                want = out_buf(d, n, 2 * h, vstep)
                lib.kernels.viz_mosaic_u8(fl, fr, sh, sw, sstep, enc, bufs["out"], h, w, MAX_DISP, want, vstep, n)
                got = d.get(viz)
                assert np.array_equal(got, d.get(want))
                p = panels(got, h, w)
                off = got_lr["mask"][:, 0] == 0
                assert off.any() and (p["bl"][off] == 0).all() and (p["br"][off] == 0).all()      # the occlusion mask shows as black
    # refusals: 2 * batch > max_batch with a check, a mask without a check, a short viz_step, a bad max_disp, a NaN tolerance, up-scaling
    f3 = d.put(pack(images(3, sh, sw, 1), capi.RT_ENC_BGR8))
    small = d.put(pack(images(2, 20, 30, 1), capi.RT_ENC_BGR8))
    bufs, viz = d.outputs(3, h, w, kind), out_buf(d, 3, 2 * h, 6 * w)
    E = capi.RT_ENC_BGR8
    for args, kw in (((f3, f3, E), dict(batch=3, src_w=sw, max_diff_px=1.0, mask=bufs["mask"], valid_count=bufs["valid_count"])),
                     ((f3, f3, E), dict(batch=2, src_w=sw, mask=bufs["mask"])),
                     ((f3, f3, E), dict(batch=2, src_w=sw, valid_count=bufs["valid_count"])),
                     ((f3, f3, E), dict(batch=2, src_w=sw, viz_step=6 * w - 1)),
                     ((f3, f3, E), dict(batch=2, src_w=sw, max_disp=0.0)),
                     ((f3, f3, E), dict(batch=2, src_w=sw, max_disp=float("nan"))),
                     ((f3, f3, E), dict(batch=2, src_w=sw, max_diff_px=float("nan"))),
                     ((f3, f3, 7), dict(batch=2, src_w=sw)),
                     ((small, small, E), dict(batch=2, src_w=30))):
        with pytest.raises(capi.RtError) as e:
            net.execute_frames_viz(args[0], args[1], args[2], bufs["out"], viz, **kw)
        got = d.read(bufs, kind)
        assert np.isnan(got["out"]).all() and (got["mask"] == 7).all() and (got["valid_count"] == 12345).all(), str(e.value)
        assert (d.get(viz) == FILL).all(), str(e.value)
    destroy()
    net.destroy()


def test_execute_frames_viz_in_graph_mode_with_rotating_buffers(rt):
    """a camera ring: three sets of frame, disparity and panel buffers in rotation on a stream and on the NULL stream with graph mode on,
    plain and checked calls alternating: the same bytes as without graphs.  (The emulator has no graphs: there the engine launches
    directly, and the rotation still runs.)"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    n, enc, kind = 2, capi.RT_ENC_BGRA8, capi.RT_DISP_PIXELS_F32
    if rt == "gpu":
        h, w, sh, sw, md = 129, 257, 376, 672, 16
    else:
        h, w, sh, sw, md = 25, 41, 51, 83, 8
    net = lib.create("resnet18_2D", w, h, max_batch=2 * n, weights=O.synth_weights_resnet18_2d(), max_disp=md)
    ring = 3 if rt == "gpu" else 2                       # (an engine pass takes seconds on the emulator)
    sets = [(d.put(pack(images(n, sh, sw, 40 + 2 * i), enc, PAD, i)), d.put(pack(images(n, sh, sw, 41 + 2 * i), enc, PAD, i + 7))) for i in range(ring)]
    vstep = 6 * w + 1

    def run(i, check, stream=None):
        bufs, viz = d.outputs(n, h, w, kind), out_buf(d, n, 2 * h, vstep)
        if rt == "gpu":
            torch.cuda.synchronize()
        net.execute_frames_viz(sets[i][0], sets[i][1], enc, bufs["out"], viz, viz_step=vstep, max_disp=MAX_DISP,
                               max_diff_px=1.0 if check else -1.0, mask=bufs["mask"] if check else None, batch=n, stream=stream, src_w=sw)
        return bufs, viz

    def read(bufs, viz):
        return d.get(bufs["out"]), d.get(bufs["mask"], np.uint8), d.get(viz)

    direct = {(i, c): read(*run(i, c)) for i in range(ring) for c in (False, True)}
    assert not np.array_equal(direct[0, False][2], direct[1, False][2]) and not np.array_equal(direct[0, False][2], direct[0, True][2])
    stream, sync, destroy, keep = make_stream(lib, rt == "gpu")
    net.set_graph(True)
    for call in range(9 if rt == "gpu" else 2):          # per engine batch: 1 direct, 2 capture + launch, then replays
        i = call % ring
        a, b = run(i, False, stream), run(i, True, stream)
        sync()
        for got, ref in ((read(*a), direct[i, False]), (read(*b), direct[i, True])):
            for x, y in zip(got, ref):
                assert np.array_equal(x, y, equal_nan=True), call
    for call in range(3 if rt == "gpu" else 1):          # and on the NULL stream, synchronously
        i = (call + 1) % ring
        for c in (False, True):
            for x, y in zip(read(*run(i, c)), direct[i, c]):
                assert np.array_equal(x, y, equal_nan=True), call
    destroy()
    net.destroy()


# ---- 6. GPU only: trained weights on the reference's sample pair -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_sample_pair_panel():
    lib, d = netlib("gpu"), Bufs(True)
    w, h = 513, 257
    net = lib.create("resnet18_2D", w, h, weights_path=model_files.weight_file("resnet18_2D"))
    left, right = sample_bgr()
    fl, fr = d.put(pack(left, capi.RT_ENC_BGR8)), d.put(pack(right, capi.RT_ENC_BGR8))
    disp, viz = d.nan(1, 1, h, w), out_buf(d, 1, 2 * h, 6 * w)
    net.execute_frames_viz(fl, fr, capi.RT_ENC_BGR8, disp, viz, max_disp=96.0, src_w=left.shape[2])
    net.destroy()
    px, p = d.get(disp), panels(d.get(viz), h, w)
    assert not np.isnan(px).any()
    for name, img in (("tl", left), ("tr", right)):
        share = frame_panel_ok(p[name], img, (h, w))
        print("sample pair %s: %.2f %% of the values within 2e-3 of a rounding tie" % (name, 100 * share))
        assert share < 0.02, share
    assert np.array_equal(p["br"], color_ref(px[:, 0], 96.0)) and np.array_equal(p["bl"], grey_ref(px[:, 0], 96.0))
    lit, positive = float((p["br"] != 0).any(axis=-1).mean()), float((px > 0).mean())
    print("sample pair: %.2f %% of the colour panel is not black, %.2f %% of the disparities are > 0" % (100 * lit, 100 * positive))
    assert abs(lit - positive) <= 0.01
