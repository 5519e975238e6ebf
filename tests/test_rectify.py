"""Raw camera frames in: rectification on the device, in front of the frame path.

- rt_rectify_maps / rt_remap_frames_u8 / rt_rectify_frames_u8: cv::initUndistortRectifyMap's model evaluated per pixel in double and
  cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) in fp32.  `positions` and `remap` restate the definition of include/rt_stereo.h in numpy, one
  rounding per operation; the kernels must equal them on the raw bits.  The restatement itself is held to its meaning by the inverse
  model (a fixed-point undistortion in float64) and by a scene rendered through it.
- rt_rectify_camera_from_info: the 3x3 inverse against numpy.
- rt_net_execute_frames_raw: one rectify launch in front of rt_net_execute_frames_3d, bit-equal to the two calls made by hand.
CPU tier: the same sources on the SIMT emulator; GPU tier (-m gpu): the MI355X, the reference's sample pair and trained weights."""
import ctypes

import numpy as np
import pytest
import torch

from redtail_amd import capi, model_files
from test_camera_frames import ENCODINGS, PAD, images, netlib, pack, rt, sample_bgr  # noqa: F401  (rt: the emu / gpu fixture)
from test_frames_any_size import NETS, NET_IDS, call_ex, outputs, read
from test_lr_consistency import Bufs, make_net
from test_points import SENTINEL, bufs_3d, call_3d, camera, compare_3d, read_points

f32, f64 = np.float32, np.float64
PIXELS, U16 = capi.RT_DISP_PIXELS_F32, capi.RT_DISP_KITTI_U16
M_F32, MM_U16 = capi.RT_DEPTH_M_F32, capi.RT_DEPTH_MM_U16
CV, DOWN = capi.RT_RESIZE_CV_AREA, capi.RT_RESIZE_AREA_DOWN
G_NET, G_FRAME = capi.RT_GEOM_NET, capi.RT_GEOM_FRAME
INF = float("inf")
ENC_IDS = ["bgr8", "rgb8", "bgra8", "rgba8"]
PLUMB_BOB = (-0.17, 0.026, 1e-3, -5e-4, 0.0)
RATIONAL = (0.3, -0.1, 1e-3, -5e-4, 0.01, 0.5, -0.05, 0.002)


# ---- the fixed rig ---------------------------------------------------------------------------------------------------------------------
def rodrigues(rx, ry, rz):
    r = np.array([rx, ry, rz], f64)
    t = np.linalg.norm(r)
    k = r / t
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], f64)
    return np.eye(3) + np.sin(t) * kx + (1 - np.cos(t)) * (kx @ kx)


def rig_info(h, w, dist=PLUMB_BOB, right=False, fx=60.0):
    """(K, D, R, P) of one camera of the rig, as a sensor_msgs/CameraInfo carries them"""
    fy, cx, cy = 0.99 * fx, (w - 1) / 2 + 1.3, (h - 1) / 2 - 0.7
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f64)
    R = rodrigues(0.01, -0.02, 0.005)
    D = np.array(dist, f64)
    if right:                                              # the sides differ: another k1, the rotation transposed
        D[0] += 0.03
        R = R.T
    P = np.zeros((3, 4), f64)
    P[:, :3] = [[0.93 * fx, 0, cx + 0.4], [0, 0.93 * fx, cy - 0.2], [0, 0, 1]]
    return K, D, R, P


def camera_np(K, D, R, P):
    """RectifyCamera without the library: the inverse by numpy (the CPU-only tests)"""
    cam = capi.RectifyCamera()
    cam.fx, cam.fy, cam.cx, cam.cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    for i, v in enumerate(np.asarray(D, f64).reshape(-1)):
        cam.d[i] = v
    for i, v in enumerate(np.linalg.inv(np.asarray(P, f64).reshape(3, 4)[:, :3] @ R).reshape(-1)):
        cam.iR[i] = v
    return cam


def rig(klib, h, w, dist=PLUMB_BOB, fx=60.0):
    """(left, right) RectifyCamera through rt_rectify_camera_from_info of the backend's library"""
    return tuple(capi.RectifyCamera.from_camera_info(*rig_info(h, w, dist, side, fx), lib=klib) for side in (False, True))


# ---- the definition restated in numpy -------------------------------------------------------------------------------------------------
def positions(cam, dh, dw):
    """the map of include/rt_stereo.h: everything in float64, every operation rounded on its own, in the order written there.  Returns
    mx, my (dh, dw) float32 and the intermediate x, y, xd, yd"""
    iR = [f64(v) for v in cam.iR]
    k1, k2, p1, p2, k3, k4, k5, k6 = (f64(v) for v in cam.d)
    fx, fy, cx, cy = f64(cam.fx), f64(cam.fy), f64(cam.cx), f64(cam.cy)
    u = np.arange(dw, dtype=f64)[None, :] + np.zeros((dh, 1), f64)
    v = np.arange(dh, dtype=f64)[:, None] + np.zeros((1, dw), f64)
    one, two = f64(1), f64(2)
    with np.errstate(all="ignore"):
        X = (iR[0] * u + iR[1] * v) + iR[2]
        Y = (iR[3] * u + iR[4] * v) + iR[5]
        W = (iR[6] * u + iR[7] * v) + iR[8]
        x, y = X / W, Y / W
        x2, y2 = x * x, y * y
        r2, xy2 = x2 + y2, (two * x) * y
        kr = (one + ((k3 * r2 + k2) * r2 + k1) * r2) / (one + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * xy2) + p2 * (r2 + two * x2)
        yd = (y * kr + p1 * (r2 + two * y2)) + p2 * xy2
        mx, my = (fx * xd + cx).astype(f32), (fy * yd + cy).astype(f32)
    assert X.dtype == f64 and kr.dtype == f64 and xd.dtype == f64
    return dict(mx=mx, my=my, x=x, y=y, xd=xd, yd=yd)


def remap(src, mx, my):
    """the sampler of include/rt_stereo.h.  src: (N, sh, sw, C) uint8, every channel alike; mx, my: (dh, dw) float32.  Returns
    ((N, dh, dw, C) uint8, the mask of the pixels whose four taps lie in the image)"""
    n, sh, sw, c = src.shape
    assert mx.dtype == f32 and my.dtype == f32
    with np.errstate(all="ignore"):
        inside = (mx > f32(-1)) & (mx < f32(sw)) & (my > f32(-1)) & (my < f32(sh))
        px, py = np.where(inside, mx, f32(0)), np.where(inside, my, f32(0))
        x0f, y0f = np.floor(px), np.floor(py)
        a, b = (px - x0f).astype(f32), (py - y0f).astype(f32)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        ua, ub = f32(1) - a, f32(1) - b

        def tap(yy, xx):
            ok = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
            val = src[:, np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1), :].astype(f32)
            return np.where(ok[None, :, :, None], val, f32(0)), ok

        (s00, k00), (s01, k01), (s10, k10), (s11, k11) = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
        a_, b_, ua_, ub_ = (t[None, :, :, None] for t in (a, b, ua, ub))
        top = s00 * ua_ + s01 * a_
        bot = s10 * ua_ + s11 * a_
        v = top * ub_ + bot * b_
        assert top.dtype == f32 and v.dtype == f32
        out = np.where(inside[None, :, :, None], np.rint(v), f32(0)).astype(np.uint8)
    return out, inside & k00 & k01 & k10 & k11


def pixels(frames, w, bpp):
    """(N, H, step) packed frames -> (N, H, w, bpp) bytes in memory order"""
    return frames[:, :, :w * bpp].reshape(frames.shape[0], frames.shape[1], w, bpp)


def expected(src_frames, sw, bpp, mx, my, pad):
    """the destination buffer as it must look: the restatement's bytes, and behind each row's last pixel the sentinel it was filled with"""
    res, _ = remap(pixels(src_frames, sw, bpp), mx, my)
    n, dh, dw, _ = res.shape
    out = np.full((n, dh, dw * bpp + pad), SENTINEL, np.uint8)
    out[:, :, :dw * bpp] = res.reshape(n, dh, dw * bpp)
    return out


def raw_pair(n, h, w, enc, pad, seed):
    return pack(images(n, h, w, seed), enc, pad, seed + 1), pack(images(n, h, w, seed + 50), enc, pad, seed + 51)


def assert_bytes(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.dtype, ref.shape)
    assert np.array_equal(got, ref), (what, int((got != ref).sum()))


# ---- 1. the definition, bit for bit ---------------------------------------------------------------------------------------------------------
SHAPES = [((37, 53), (37, 53)), ((45, 77), (45, 77)), ((45, 77), (29, 131))]


@pytest.mark.parametrize("pad", [0, PAD], ids=["dense", "pitched"])
@pytest.mark.parametrize("enc", ENCODINGS, ids=ENC_IDS)
@pytest.mark.parametrize("src,dst", SHAPES, ids=["%dx%d-%dx%d" % (s[1], s[0], t[1], t[0]) for s, t in SHAPES])
def test_bit_equal_to_restatement(backend, src, dst, enc, pad):
    """rt_rectify_maps on the raw bits of the maps; rt_remap_frames_u8 and rt_rectify_frames_u8 on the raw bytes, and equal to each other;
    batch 1 and 2, plumb_bob and rational_polynomial taking turns; the bytes behind each row's end keep their sentinel.  131 columns
    cross two 64-column blocks, 29 and 37 rows are no multiple of 4, the pitched rows of the 4-byte encodings are off a dword."""
    d, k = Bufs(backend.name == "gpu"), backend.klib
    (sh, sw), (dh, dw) = src, dst
    bpp = capi.ENC_BYTES[enc]
    for n in (1, 2):
        dist = PLUMB_BOB if (n + enc) % 2 else RATIONAL
        cl, cr = rig(k, sh, sw, dist)
        fl, fr = raw_pair(n, sh, sw, enc, pad, seed=7 * n + enc)
        maps, refs = [], []
        for cam in (cl, cr):
            ref = positions(cam, dh, dw)
            mxy = d.full((dh, dw), f32, -7.0), d.full((dh, dw), f32, -7.0)
            k.rectify_maps(cam, dh, dw, *mxy)
            assert_bytes(d.get(mxy[0]).view(np.uint32), ref["mx"].view(np.uint32), "map x")
            assert_bytes(d.get(mxy[1]).view(np.uint32), ref["my"].view(np.uint32), "map y")
            maps += list(mxy)
            refs.append(ref)
        want = [expected(f, sw, bpp, r["mx"], r["my"], pad) for f, r in zip((fl, fr), refs)]
        assert all(0.3 < (w_[:, :, :dw * bpp] != 0).mean() for w_ in want)
        dstep = dw * bpp + pad
        by_map = d.full((n, dh, dstep), np.uint8, SENTINEL), d.full((n, dh, dstep), np.uint8, SENTINEL)
        k.remap_frames_u8(d.put(fl), d.put(fr), sh, sw, fl.shape[2], enc, *maps, *by_map, dh, dw, dstep, n)
        direct = d.full((n, dh, dstep), np.uint8, SENTINEL), d.full((n, dh, dstep), np.uint8, SENTINEL)
        k.rectify_frames_u8(d.put(fl), d.put(fr), sh, sw, fl.shape[2], enc, cl, cr, *direct, dh, dw, dstep, n)
        for side in (0, 1):
            assert_bytes(d.get(by_map[side]), want[side], ("remap", n, side))
            assert_bytes(d.get(direct[side]), want[side], ("rectify", n, side))
        assert want[0].tobytes() != want[1].tobytes()


# ---- 2. positions the sampler must survive -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", [capi.RT_ENC_BGR8, capi.RT_ENC_RGBA8], ids=["bgr8", "rgba8"])
def test_special_positions_follow_the_restatement(backend, enc):
    """NaN, +-inf, +-1e30, -1, -0.5, 0, n-1, n-0.5, n in x and in y, every combination of them and each beside an ordinary position,
    scattered over a 9 x 70 destination: 0 where not inside, half-weight blends with the border's 0 at the +-0.5 positions.  A camera whose
    iR has a last row of 0 makes every W 0 and every position non-finite: the frame is all 0."""
    d, k = Bufs(backend.name == "gpu"), backend.klib
    sh, sw, dh, dw, n = 12, 20, 9, 70, 2
    bpp = capi.ENC_BYTES[enc]
    nan = float("nan")
    rng = np.random.default_rng(5)
    maps = []
    for side in (0, 1):
        mx = rng.uniform(-2, sw + 1, (dh, dw)).astype(f32)
        my = rng.uniform(-2, sh + 1, (dh, dw)).astype(f32)
        xs = [nan, INF, -INF, 1e30, -1e30, -1.0, -0.5, 0.0, sw - 1, sw - 0.5, sw, 3.25]
        ys = [nan, INF, -INF, 1e30, -1e30, -1.0, -0.5, 0.0, sh - 1, sh - 0.5, sh, 4.75]
        where = rng.permutation(dh * dw)[:len(xs) * len(ys)]
        for i, o in enumerate(where):
            mx.flat[o], my.flat[o] = xs[i % len(xs)], ys[i // len(xs)]
        maps += [mx, my]
    fl, fr = raw_pair(n, sh, sw, enc, PAD, seed=60)
    dstep = dw * bpp + PAD
    out = d.full((n, dh, dstep), np.uint8, SENTINEL), d.full((n, dh, dstep), np.uint8, SENTINEL)
    k.remap_frames_u8(d.put(fl), d.put(fr), sh, sw, fl.shape[2], enc, *(d.put(m) for m in maps), *out, dh, dw, dstep, n)
    for side, f in enumerate((fl, fr)):
        assert_bytes(d.get(out[side]), expected(f, sw, bpp, maps[2 * side], maps[2 * side + 1], PAD), side)
    # the restatement where it can be read off by hand (ties go to even, as rintf)
    src = pixels(fl, sw, bpp)
    at = lambda x, y: remap(src, np.full((1, 1), x, f32), np.full((1, 1), y, f32))[0][:, 0, 0, :]
    half = lambda a: np.rint(a.astype(f32) * f32(0.5)).astype(np.uint8)
    assert np.array_equal(at(0.0, 0.0), src[:, 0, 0]) and np.array_equal(at(sw - 1, sh - 1), src[:, sh - 1, sw - 1])
    assert np.array_equal(at(-0.5, 0.0), half(src[:, 0, 0])) and np.array_equal(at(sw - 0.5, 2.0), half(src[:, 2, sw - 1]))
    assert np.array_equal(at(3.0, -0.5), half(src[:, 0, 3])) and np.array_equal(at(3.0, sh - 0.5), half(src[:, sh - 1, 3]))
    for x, y in ((-1.0, 3.0), (sw, 3.0), (3.0, -1.0), (3.0, sh), (nan, 3.0), (3.0, nan), (INF, 3.0), (3.0, -INF), (1e30, 3.0), (-1e30, -1e30)):
        assert (at(x, y) == 0).all(), (x, y)
    # every W is 0: X / W and Y / W are infinities and NaNs
    cam = capi.RectifyCamera.from_camera_info(*rig_info(sh, sw), lib=k)
    for i in (6, 7, 8):
        cam.iR[i] = 0.0
    ref = positions(cam, dh, dw)
    assert not np.isfinite(ref["mx"]).any() and not np.isfinite(ref["my"]).any()
    out = d.full((n, dh, dstep), np.uint8, SENTINEL), d.full((n, dh, dstep), np.uint8, SENTINEL)
    k.rectify_frames_u8(d.put(fl), d.put(fr), sh, sw, fl.shape[2], enc, cam, cam, *out, dh, dw, dstep, n)
    for o in out:
        got = d.get(o)
        assert (got[:, :, :dw * bpp] == 0).all() and (got[:, :, dw * bpp:] == SENTINEL).all()


# ---- 3. identity and shift ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ENCODINGS, ids=ENC_IDS)
def test_identity_and_whole_pixel_shift(backend, enc):
    d, k = Bufs(backend.name == "gpu"), backend.klib
    h, w, n = 37, 53, 2
    bpp = capi.ENC_BYTES[enc]
    K = rig_info(h, w)[0]
    P = np.zeros((3, 4))
    P[:, :3] = K
    ident = capi.RectifyCamera.from_camera_info(K, None, np.eye(3), P, lib=k)
    P[0, 2] += 3
    P[1, 2] -= 2
    shift = capi.RectifyCamera.from_camera_info(K, [0.0] * 5, np.eye(3), P, lib=k)
    fl, fr = raw_pair(n, h, w, enc, PAD, seed=70)
    out = d.full((n, h, w * bpp), np.uint8, SENTINEL), d.full((n, h, w * bpp), np.uint8, SENTINEL)
    k.rectify_frames_u8(d.put(fl), d.put(fr), h, w, fl.shape[2], enc, ident, shift, *out, h, w, w * bpp, n)
    assert_bytes(d.get(out[0]).reshape(n, h, w, bpp), pixels(fl, w, bpp), "identity")
    want = np.zeros((n, h, w, bpp), np.uint8)                # rectified (v, u) looks at raw (v + 2, u - 3)
    want[:, :h - 2, 3:] = pixels(fr, w, bpp)[:, 2:, :w - 3]
    assert_bytes(d.get(out[1]).reshape(n, h, w, bpp), want, "shift")


# ---- 4. the restatement means what it says --------------------------------------------------------------------------------------------------------
def undistort(cam, xd, yd, steps=50):
    """the usual fixed-point iteration (cv::undistortPoints) in float64: normalised distorted -> normalised ideal"""
    k1, k2, p1, p2, k3, k4, k5, k6 = (f64(v) for v in cam.d)
    x, y = xd.copy(), yd.copy()
    for _ in range(steps):
        r2 = x * x + y * y
        icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) * icdist, (yd - dy) * icdist
    return x, y


@pytest.mark.parametrize("dist", [PLUMB_BOB, RATIONAL], ids=["plumb_bob", "rational"])
def test_restatement_inverts_through_the_undistortion(dist):
    """(a) undistorting the restatement's (xd, yd) returns its (x, y) to within 1e-9 px (the error times fx)"""
    for (h, w), fx in (((45, 77), 60.0), ((720, 1280), 700.0)):
        for right in (False, True):
            cam = camera_np(*rig_info(h, w, dist, right, fx))
            p = positions(cam, h, w)
            x, y = undistort(cam, p["xd"], p["yd"])
            err = max(np.abs(x - p["x"]).max() * cam.fx, np.abs(y - p["y"]).max() * cam.fy)
            print("%dx%d %s: undistortion returns the ideal point to %.2g px" % (w, h, "right" if right else "left", err))
            assert err <= 1e-9, err


def scene(u, v):
    return 127.5 + 100.0 * np.sin(2 * np.pi * u / 24.0) * np.cos(2 * np.pi * v / 31.2)


def render_raw(info, h, w):
    """the grey scene, defined on the rectified image, as the raw camera sees it: every raw pixel through the inverse model, in float64;
    (1, h, w, 3) uint8, the three channels alike"""
    K, D, R, P = info
    cam = camera_np(K, D, R, P)
    i, j = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    x, y = undistort(cam, (i - cam.cx) / cam.fx, (j - cam.cy) / cam.fy)
    m = P[:, :3] @ R
    uvw = m @ np.stack([x.ravel(), y.ravel(), np.ones(h * w)])
    u, v = (uvw[0] / uvw[2]).reshape(h, w), (uvw[1] / uvw[2]).reshape(h, w)
    grey = np.rint(np.clip(scene(u, v), 0, 255)).astype(np.uint8)
    return np.repeat(grey[None, :, :, None], 3, axis=3)


def check_scene(rect, full, what):
    """a rectified (h, w, 3) picture against the scene itself, on the pixels whose four taps lay in the raw image.
    Bound: the bilinear error of f is at most (|f_uu| + |f_vv|) / 8 = 100 * ((2 pi / 24)^2 + (2 pi / 31.2)^2) / 8 = 1.37 grey levels in
    raw pixels of about the rectified size, plus two roundings to a byte (the rendering's and the sampler's) of 0.5 each: 3 at most; the
    mean of that chain is bounded by 0.75.  At least 90 % of the picture must take part."""
    h, w = full.shape
    u, v = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    err = np.abs(rect[..., 0].astype(f64) - scene(u, v))[full]
    assert (rect[..., 0] == rect[..., 1]).all() and (rect[..., 0] == rect[..., 2]).all()
    print("%s: max error %.2f, mean %.2f grey levels over %.1f %% of the picture" % (what, err.max(), err.mean(), 100.0 * full.mean()))
    assert full.mean() >= 0.9, full.mean()
    assert err.max() <= 3.0 and err.mean() <= 0.75, (what, err.max(), err.mean())


@pytest.mark.parametrize("dist", [PLUMB_BOB, RATIONAL], ids=["plumb_bob", "rational"])
def test_restatement_recovers_a_rendered_scene(dist):
    """(b) restatement only: 2.09 / 0.49 (plumb_bob) and 2.14 / 0.52 (rational) grey levels max / mean over 94.6 % / 95.9 %"""
    h, w = 45, 77
    info = rig_info(h, w, dist)
    raw = render_raw(info, h, w)
    p = positions(camera_np(*info), h, w)
    rect, full = remap(raw, p["mx"], p["my"])
    check_scene(rect[0], full, "restatement")


@pytest.mark.parametrize("dist", [PLUMB_BOB, RATIONAL], ids=["plumb_bob", "rational"])
def test_kernel_recovers_a_rendered_scene(backend, dist):
    """... and the same comparison through rt_rectify_frames_u8, which inherits the bound because it is bit-equal"""
    d, k = Bufs(backend.name == "gpu"), backend.klib
    h, w = 45, 77
    info = rig_info(h, w, dist)
    raw = render_raw(info, h, w)
    cam = capi.RectifyCamera.from_camera_info(*info, lib=k)
    p = positions(cam, h, w)
    ref, full = remap(raw, p["mx"], p["my"])
    frames = d.put(raw.reshape(1, h, 3 * w))
    out = d.full((1, h, 3 * w), np.uint8, SENTINEL), d.full((1, h, 3 * w), np.uint8, SENTINEL)
    k.rectify_frames_u8(frames, frames, h, w, 3 * w, capi.RT_ENC_BGR8, cam, cam, *out, h, w, 3 * w, 1)
    got = d.get(out[0]).reshape(1, h, w, 3)
    assert_bytes(got, ref)
    assert_bytes(d.get(out[1]).reshape(1, h, w, 3), ref)
    check_scene(got[0], full, "kernel")


# ---- 5. rt_rectify_camera_from_info --------------------------------------------------------------------------------------------------------------
def test_camera_from_info(backend):
    k = backend.klib
    for dist, right in ((PLUMB_BOB, False), (RATIONAL, True)):
        K, D, R, P = rig_info(45, 77, dist, right)
        for n_d in (0, 4, 5, 8):
            coeff = list(D[:n_d]) + [0.1, 0.2, 0.3][:max(0, n_d - len(D))]
            cam = capi.RectifyCamera.from_camera_info(K, coeff, R, P, lib=k)
            want = np.linalg.inv(P[:, :3] @ R).reshape(-1)
            got = np.array(list(cam.iR))
            assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), np.abs(got - want) / np.abs(want)
            assert (cam.fx, cam.fy, cam.cx, cam.cy) == (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
            assert list(cam.d) == coeff + [0.0] * (8 - n_d)
    K, D, R, P = rig_info(45, 77)
    bad_k = K.copy()
    bad_k[1, 2] = np.nan
    bad_p = P.copy()
    bad_p[:, :3] = 0
    for args in ((K, list(D[:3]), R, P), (bad_k, D, R, P), (K, D, R, bad_p), (K, [np.inf] * 5, R, P), (K, D, R * np.nan, P)):
        with pytest.raises(capi.RtError):
            capi.RectifyCamera.from_camera_info(*args, lib=k)


# ---- 6. the net call is its composition -------------------------------------------------------------------------------------------------------------
def call_raw(net, fl, fr, enc, cl, cr, cam, b, n, resize, max_diff, zmin=0.0, zmax=INF, depth_kind=M_F32, disp_kind=PIXELS, **kw):
    net.execute_frames_raw(fl, fr, enc, cl, cr, cam, disp=b["disp"], kind=disp_kind, resize=resize, max_diff_px=max_diff, mask=b["mask"],
                           valid_count=b["valid_count"], min_depth=zmin, max_depth=zmax, depth=b["depth"], depth_kind=depth_kind,
                           points=b["points"], points_compact=b["compact"], count=b["count"], batch=n, **kw)


def rectify_by_hand(k, d, fl, fr, sh, sw, enc, cl, cr, n, pad=0):
    bpp = capi.ENC_BYTES[enc]
    out = d.full((n, sh, sw * bpp + pad), np.uint8, SENTINEL), d.full((n, sh, sw * bpp + pad), np.uint8, SENTINEL)
    k.rectify_frames_u8(fl, fr, sh, sw, fl.shape[2], enc, cl, cr, *out, sh, sw, sw * bpp + pad, n)
    return out


ALL = ("depth", "points", "compact")


@pytest.mark.parametrize("model,flags", NETS, ids=NET_IDS)
def test_execute_frames_raw_equals_the_two_calls_by_hand(rt, model, flags):
    """rt_net_execute_frames_raw against rt_rectify_frames_u8 into dense buffers followed by rt_net_execute_frames_3d on them: disparity
    (16-bit; fp32 below), mask, count, depth, organised and compact cloud, bit for bit, with a check, into the caller's pitched rectified
    buffers, which then hold the op's output.  Then larger frames without a check and with out == NULL, into the net's own buffers:
    rt_net_execute_frames_ex on the rectified frames, which the same net runs between the two raw calls.  (An engine pass on the
    emulator takes seconds, so the cases share passes: every raw call has one counterpart by hand.)"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    net, h, w, scale = make_net(lib, model, flags)
    n, enc = (2 if flags else 1), capi.RT_ENC_BGRA8
    bpp = 4
    modes = [(CV, 1.5, 30, 36, MM_U16, U16), (DOWN, -1.0, 51, 83, M_F32, PIXELS)]
    for i, (resize, max_diff, sh, sw, depth_kind, disp_kind) in enumerate(modes):
        check = max_diff >= 0
        cl, cr = rig(k, sh, sw, RATIONAL if i % 2 else PLUMB_BOB, fx=40.0)
        raw_l, raw_r = raw_pair(n, sh, sw, enc, PAD, seed=80 + i)
        fl, fr = d.put(raw_l), d.put(raw_r)
        cam = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)
        zmin, zmax = ((0.0, INF), (0.05, 1.0))[i % 2]
        rl, rr = rectify_by_hand(k, d, fl, fr, sh, sw, enc, cl, cr, n)
        assert d.get(rl).tobytes() != d.get(rr).tobytes() and (d.get(rl) != 0).mean() > 0.5
        if check:
            b = bufs_3d(d, n, sh, sw, True, ALL, check, depth_kind, disp_kind)
            call_3d(net, rl, rr, enc, cam, b, n, resize, max_diff, zmin, zmax, depth_kind, disp_kind, src_w=sw)
            ref = read_points(d, b, disp_kind, depth_kind)
            assert 0 < ref["count"].sum() <= n * sh * sw
            b = bufs_3d(d, n, sh, sw, True, ALL, check, depth_kind, disp_kind)
            kw = dict(left_rect=d.full((n, sh, sw * bpp + PAD), np.uint8, SENTINEL), right_rect=d.full((n, sh, sw * bpp + PAD), np.uint8, SENTINEL))
            call_raw(net, fl, fr, enc, cl, cr, cam, b, n, resize, max_diff, zmin, zmax, depth_kind, disp_kind, src_w=sw, **kw)
            compare_3d(read_points(d, b, disp_kind, depth_kind), ref, n, sh * sw, (i, "raw"))
            want = rectify_by_hand(k, d, fl, fr, sh, sw, enc, cl, cr, n, PAD)           # the caller's buffers, rows PAD bytes longer than the pixels
            assert_bytes(d.get(kw["left_rect"]), d.get(want[0]), "left_rect")
            assert_bytes(d.get(kw["right_rect"]), d.get(want[1]), "right_rect")
            assert (d.get(kw["left_rect"])[:, :, sw * bpp:] == SENTINEL).all()
            continue
        # out == NULL is rt_net_execute_frames_ex on the rectified frames; the same net runs that call between two raw ones
        old = read(d, call_ex(d, net, rl, rr, enc, n, sh, sw, PIXELS, G_FRAME, resize, max_diff, src_w=sw), PIXELS)
        new = outputs(d, n, sh, sw, PIXELS)
        net.execute_frames_raw(fl, fr, enc, cl, cr, None, disp=new["out"], resize=resize, max_diff_px=max_diff, mask=new["mask"] if check else None,
                               valid_count=new["valid_count"] if check else None, batch=n, src_w=sw, no_depth_call=True)
        new = read(d, new, PIXELS)
        for key in old:
            assert np.array_equal(new[key], old[key]), (i, key)
    net.destroy()


def raw_outputs(d, n, sh, sw, bpp):
    b = bufs_3d(d, n, sh, sw, True, ALL, True)
    b["left_rect"] = d.full((n, sh, sw * bpp + PAD), np.uint8, SENTINEL)
    b["right_rect"] = d.full((n, sh, sw * bpp + PAD), np.uint8, SENTINEL)
    return b


def raw_untouched(d, b):
    g = read_points(d, {key: v for key, v in b.items() if "rect" not in key}, PIXELS, M_F32)
    return (np.isnan(g["disp"]).all() and (g["mask"] == 7).all() and (g["valid_count"] == 12345).all() and
            (g["depth"] == f32(1e30).view(np.uint32)).all() and (g["points"].view(np.uint8) == SENTINEL).all() and
            (g["compact"].view(np.uint8) == SENTINEL).all() and (g["count"] == 12345).all() and
            (d.get(b["left_rect"]) == SENTINEL).all() and (d.get(b["right_rect"]) == SENTINEL).all())


# ---- 7. refusals write nothing ----------------------------------------------------------------------------------------------------------------------
def test_op_refusals(backend):
    d, k = Bufs(backend.name == "gpu"), backend.klib
    sh, sw, dh, dw, enc, bpp = 20, 30, 16, 24, capi.RT_ENC_BGRA8, 4
    cl, cr = rig(k, sh, sw)
    fl, fr = (d.put(f) for f in raw_pair(1, sh, sw, enc, 0, seed=90))
    out = d.full((1, dh, dw * bpp), np.uint8, SENTINEL), d.full((1, dh, dw * bpp), np.uint8, SENTINEL)
    maps = [d.full((dh, dw), f32, 2.0) for _ in range(4)]
    bad_cam = capi.RectifyCamera.from_camera_info(*rig_info(sh, sw), lib=k)
    bad_cam.d[6] = float("nan")
    inf_cam = capi.RectifyCamera.from_camera_info(*rig_info(sh, sw), lib=k)
    inf_cam.iR[2] = INF

    def args(**kw):
        a = dict(left=fl, right=fr, sh=sh, sw=sw, step=sw * bpp, enc=enc, cl=cl, cr=cr, dl=out[0], dr=out[1], dh=dh, dw=dw, dstep=dw * bpp, n=1)
        a.update(kw)
        return a

    def rectify(a):
        k.rectify_frames_u8(a["left"], a["right"], a["sh"], a["sw"], a["step"], a["enc"], a["cl"], a["cr"], a["dl"], a["dr"], a["dh"], a["dw"],
                            a["dstep"], a["n"])

    def remap_(a):
        k.remap_frames_u8(a["left"], a["right"], a["sh"], a["sw"], a["step"], a["enc"], *a.get("maps", maps), a["dl"], a["dr"], a["dh"], a["dw"],
                          a["dstep"], a["n"])

    same = d.full((1, sh, sw * bpp), np.uint8, SENTINEL)
    common = [dict(enc=4), dict(enc=-1), dict(step=sw * bpp - 1), dict(dstep=dw * bpp - 1), dict(step=sw * 3 - 1, enc=capi.RT_ENC_BGR8),
              dict(sh=0), dict(sw=0), dict(dh=0), dict(dw=0), dict(n=0), dict(left=None), dict(right=None), dict(dl=None), dict(dr=None),
              dict(left=same, dl=same, dh=sh, dw=sw, dstep=sw * bpp), dict(right=same, dr=same, dh=sh, dw=sw, dstep=sw * bpp)]
    for fn, cases in ((rectify, common + [dict(cl=bad_cam), dict(cr=bad_cam), dict(cl=inf_cam), dict(cl=None), dict(cr=None)]),
                      (remap_, common + [dict(maps=[maps[0], None, maps[2], maps[3]])])):
        for kw in cases:
            with pytest.raises(capi.RtError):
                fn(args(**kw))
            assert all((d.get(o) == SENTINEL).all() for o in out + (same,)), (fn.__name__, kw)
        fn(args())                                         # and next to them it works
        assert not (d.get(out[0]) == SENTINEL).all()
        for o in out:
            o[...] = SENTINEL
    mx = d.full((dh, dw), f32, -7.0)
    for cam, hh, ww in ((bad_cam, dh, dw), (None, dh, dw), (cl, 0, dw), (cl, dh, 0)):
        with pytest.raises(capi.RtError):
            k.rectify_maps(cam, hh, ww, mx, mx)
        assert (d.get(mx) == -7.0).all()


@pytest.mark.parametrize("model,flags", NETS[1:2], ids=NET_IDS[1:2])
def test_net_refusals_write_nothing(rt, model, flags):
    """what only the new struct can get wrong, and refusals of the wrapped call reached through the new one: an error, sentinel-filled
    outputs -- the caller's rectified frames among them -- untouched"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    net, h, w, scale = make_net(lib, model, flags)
    n, enc, bpp, sh, sw = 1, capi.RT_ENC_BGRA8, 4, 30, 36
    cl, cr = rig(k, sh, sw, fx=40.0)
    fl, fr = (d.put(f) for f in raw_pair(n, sh, sw, enc, 0, seed=95))
    cam = camera(fx=30.0, fy=31.0, cx=18.0, cy=15.0, baseline=0.1)
    b = raw_outputs(d, n, sh, sw, bpp)
    nan = float("nan")
    bad_cam = capi.RectifyCamera.from_camera_info(*rig_info(sh, sw), lib=k)
    bad_cam.cy = nan
    big_l, big_r = (d.put(f) for f in raw_pair(5, sh, sw, enc, 0, seed=96))
    small = d.put(raw_pair(n, 20, 30, enc, 0, seed=97)[0])      # the down-only filter refuses it: both axes would grow
    small_rect = d.full((n, 20, 30 * bpp + PAD), np.uint8, SENTINEL)
    bad = [dict(rect_struct_bytes=ctypes.sizeof(capi.RectifyCall) - 8), dict(rect_struct_bytes=0),
           dict(right_rect=None), dict(left_rect=None), dict(rect_step=sw * bpp - 1), dict(left_rect=None, right_rect=None, rect_step=sw * bpp),
           dict(cl=bad_cam), dict(cr=bad_cam), dict(left_rect=fl), dict(right_rect=fr),
           dict(geometry=G_NET), dict(struct_bytes=ctypes.sizeof(capi.FrameCall) - 8), dict(depth_struct_bytes=0), dict(resize=2), dict(geometry=2),
           dict(disp_kind=3), dict(disp_kind=capi.RT_DISP_NET), dict(depth_kind=2), dict(max_diff=nan), dict(cam=camera(fx=0.0)),
           dict(cam=camera(doffs=nan)), dict(zmin=2.0, zmax=1.0), dict(batch=3, fl=big_l, fr=big_r), dict(batch=0), dict(src_step=sw * bpp - 1),
           dict(resize=DOWN, fl=small, fr=small, left_rect=small_rect, right_rect=small_rect)]
    for kw in bad:
        kw = dict(kw)
        a = dict(resize=CV, max_diff=1.5, cam=cam, fl=fl, fr=fr, batch=n, cl=cl, cr=cr, left_rect=b["left_rect"], right_rect=b["right_rect"])
        for key in list(a):
            if key in kw:
                a[key] = kw.pop(key)
        with pytest.raises(capi.RtError) as e:
            call_raw(net, a["fl"], a["fr"], enc, a["cl"], a["cr"], a["cam"], b, a["batch"], a["resize"], a["max_diff"],
                     src_w=30 if a["fl"] is small else sw, left_rect=a["left_rect"], right_rect=a["right_rect"], **kw)
        assert "rt_net_execute_frames_raw" in str(e.value), str(e.value)
        assert raw_untouched(d, b) and (d.get(small_rect) == SENTINEL).all(), kw
    with pytest.raises(capi.RtError):                       # compact without count
        bb = dict(b, count=None)
        call_raw(net, fl, fr, enc, cl, cr, cam, bb, n, CV, 1.5, src_w=sw, left_rect=b["left_rect"], right_rect=b["right_rect"])
    assert raw_untouched(d, b)
    call_raw(net, fl, fr, enc, cl, cr, cam, b, n, CV, 1.5, src_w=sw, left_rect=b["left_rect"], right_rect=b["right_rect"])       # and the valid call works
    assert not raw_untouched(d, b) and not (d.get(b["left_rect"])[:, :, :sw * bpp] == SENTINEL).all()
    net.destroy()


# ---- 8. GPU only: the reference's sample pair and trained weights; graph mode ---------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_sample_pair_as_raw_frames_and_graph_mode():
    """ResNet-18 2D 1257 x 369 fp32, trained weights, the reference's 1242 x 375 pair treated as raw frames of a rig with fx = 700: the raw
    call equals the two calls by hand on every output, with a check; the cloud's colour is the rectified left pixel; then graph mode on a
    stream with three sets of frame and output buffers in rotation, each rotation bit-equal to the direct result"""
    lib, d = netlib("gpu"), Bufs(True)
    k = lib.kernels
    w, h = 1257, 369
    net = lib.create("resnet18_2D", w, h, max_batch=2, weights_path=model_files.weight_file("resnet18_2D"))
    left, right = sample_bgr()
    sh, sw = left.shape[1:3]
    enc = capi.RT_ENC_BGR8
    cl, cr = rig(k, sh, sw, fx=700.0)
    cam = camera(fx=0.93 * 700.0, fy=0.93 * 700.0, cx=float(cl.cx) + 0.4, cy=float(cl.cy) - 0.2, baseline=0.54)
    sets = [(d.put(pack(np.roll(left, 7 * i, axis=2), enc, PAD)), d.put(pack(np.roll(right, 7 * i, axis=2), enc, PAD))) for i in range(3)]
    direct = []
    for i, (fl, fr) in enumerate(sets):
        rl, rr = rectify_by_hand(k, d, fl, fr, sh, sw, enc, cl, cr, 1)
        b = bufs_3d(d, 1, sh, sw, True, ALL, True)
        call_3d(net, rl, rr, enc, cam, b, 1, CV, 1.0, 0.5, 80.0, src_w=sw)
        direct.append(read_points(d, b, PIXELS, M_F32))
        if i == 0:
            pts = direct[0]["points"].reshape(sh, sw, 4)
            rect = d.get(rl).reshape(sh, sw, 3).astype(np.uint32)
            assert np.array_equal(pts[..., 3], (rect[..., 2] << 16) | (rect[..., 1] << 8) | rect[..., 0])
            assert 0 < direct[0]["count"][0] < sh * sw
    assert direct[0]["points"].tobytes() != direct[1]["points"].tobytes()
    for i, (fl, fr) in enumerate(sets):
        b = bufs_3d(d, 1, sh, sw, True, ALL, True)
        call_raw(net, fl, fr, enc, cl, cr, cam, b, 1, CV, 1.0, 0.5, 80.0, src_w=sw)
        compare_3d(read_points(d, b, PIXELS, M_F32), direct[i], 1, sh * sw, ("direct", i))
    net.set_graph(True)
    s = torch.cuda.Stream()
    for call in range(7):                                  # 1: direct, 2: capture + launch, then replays, whatever pointers rotate in
        i = call % 3
        b = bufs_3d(d, 1, sh, sw, True, ALL, True)
        rects = dict(left_rect=d.full((1, sh, sw * 3 + PAD), np.uint8, SENTINEL), right_rect=d.full((1, sh, sw * 3 + PAD), np.uint8, SENTINEL)) if call % 2 else {}
        torch.cuda.synchronize()
        call_raw(net, sets[i][0], sets[i][1], enc, cl, cr, cam, b, 1, CV, 1.0, 0.5, 80.0, src_w=sw, stream=s.cuda_stream, **rects)
        s.synchronize()
        compare_3d(read_points(d, b, PIXELS, M_F32), direct[i], 1, sh * sw, ("graph", call))
    net.destroy()
