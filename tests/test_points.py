"""Depth and a point cloud out of the camera-frame path.

- rt_disparity_to_points: rt_disparity_to_frame's resampling followed, in one launch, by the reprojection of a rectified pair: depth image
  (REP 118, fp32 metres or uint16 millimetres), organised cloud of 16-byte {x, y, z, rgb} records, and -- one more launch -- the compact
  cloud of the valid points with its count.  `to_points` restates the definition in numpy float32, one rounding per operation; the kernel
  must equal it on the raw bytes, NaN patterns included.  The restatement itself is held to its meaning by an fp64 evaluation of the
  three formulas on planes with known equations.
- rt_net_execute_frames_3d: the op behind one engine pass, bit-equal to the op-level calls made by hand around rt_net_execute.
CPU tier: the same sources on the SIMT emulator; GPU tier (-m gpu): the MI355X, the reference's sample pair and trained weights."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from oracle import stereo_oracle as O
from redtail_amd import capi, model_files
from test_camera_frames import ENCODINGS, PAD, images, netlib, pack, rt, sample_bgr  # noqa: F401  (rt: the emu / gpu fixture)
from test_frames_any_size import NETS, NET_IDS, call_ex, disparity_field, engine_by_hand, outputs, read, run_to_frame, to_frame
from test_lr_consistency import Bufs, make_net

f32, u32 = np.float32, np.uint32
PIXELS, U16 = capi.RT_DISP_PIXELS_F32, capi.RT_DISP_KITTI_U16
M_F32, MM_U16 = capi.RT_DEPTH_M_F32, capi.RT_DEPTH_MM_U16
CV, DOWN = capi.RT_RESIZE_CV_AREA, capi.RT_RESIZE_AREA_DOWN
G_NET, G_FRAME = capi.RT_GEOM_NET, capi.RT_GEOM_FRAME
NAN_BITS = u32(0x7FC00000)
INF = float("inf")
SENTINEL = 0xA5                                            # byte the clouds are pre-filled with


def camera(fx=700.0, fy=690.0, cx=20.25, cy=11.5, baseline=0.12, doffs=0.0):
    return capi.StereoCamera(fx, fy, cx, cy, baseline, doffs)


# ---- the definition restated in numpy -------------------------------------------------------------------------------------------------
def to_points(px, mask, fh, fw, cam, zmin, zmax, rgb=None):
    """what rt_disparity_to_points must write, bit for bit.  px: (N,1,H,W) float32, mask: (N,1,H,W) uint8 or None, rgb: (N,fh,fw) uint32
    R << 16 | G << 8 | B or None.  Returns the raw bits: depth_m / depth_mm (N,1,fh,fw), points (N,fh,fw,4) uint32, ok (N,fh,fw) bool,
    compact (list of (count, 4) uint32 per image), count (N,) uint64."""
    fr = to_frame(px, mask, fh, fw, PIXELS)
    v = fr["out"][:, 0]                                       # 0 where not valid0: such a pixel is not ok whatever its value
    valid0 = fr["mask"][:, 0] != 0 if mask is not None else np.ones(v.shape, bool)
    fx, fy, cx, cy, doffs = f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy), f32(cam.doffs)
    fB = f32(fx * f32(cam.baseline))                          # formed once, in fp32
    zmin, zmax = f32(zmin), f32(zmax)
    with np.errstate(all="ignore"):
        den = (v + doffs).astype(f32)
        ok = valid0 & (den > 0) & np.isfinite(den)
        Z = (fB / den).astype(f32)
        ok = ok & (Z >= zmin) & (Z <= zmax)
        u = np.arange(fw, dtype=f32)[None, None, :]
        r = np.arange(fh, dtype=f32)[None, :, None]
        X = (((u - cx).astype(f32) / fx).astype(f32) * Z).astype(f32)
        Y = (((r - cy).astype(f32) / fy).astype(f32) * Z).astype(f32)
        q = np.rint((Z * f32(1000)).astype(f32))
        q = np.where(q > 0, np.minimum(q, f32(65535)), f32(0))  # a NaN: 0
        mm = np.maximum(q.astype(np.uint16), 1)
    assert Z.dtype == f32 and X.dtype == f32 and Y.dtype == f32
    nan = np.full(Z.shape, NAN_BITS, u32)
    col = np.zeros(Z.shape, u32) if rgb is None else rgb.astype(u32)
    pts = np.stack([np.where(ok, X.view(u32), nan), np.where(ok, Y.view(u32), nan), np.where(ok, Z.view(u32), nan), col], axis=-1)
    return dict(depth_m=np.where(ok, Z.view(u32), nan)[:, None], depth_mm=np.where(ok, mm, np.uint16(0))[:, None], points=pts, ok=ok,
                compact=[pts[i][ok[i]] for i in range(len(pts))], count=ok.sum(axis=(1, 2)).astype(np.uint64))


def rgb_of(bgr):
    """(N,H,W,3) BGR uint8 -> (N,H,W) uint32 R << 16 | G << 8 | B"""
    b = bgr.astype(u32)
    return (b[..., 2] << 16) | (b[..., 1] << 8) | b[..., 0]


def run_points(klib, d, px, mask, fh, fw, cam, zmin=0.0, zmax=INF, frames=None, encoding=capi.RT_ENC_BGR8, disp_kind=None, depth_kind=None,
               points=False, compact=False, count=False, want_mask=False, want_vcount=False, bufs=None, stream=None):
    """one call with sentinel-filled outputs; returns (raw arrays read back, the buffers)"""
    n, _, h, w = px.shape
    if bufs is None:
        bufs = {}
        if disp_kind is not None:
            bufs["disp"] = d.full((n, 1, fh, fw), np.uint16, 0xFFFF) if disp_kind == U16 else d.nan(n, 1, fh, fw)
        if depth_kind is not None:
            bufs["depth"] = d.full((n, 1, fh, fw), np.uint16, 0xFFFF) if depth_kind == MM_U16 else d.full((n, 1, fh, fw), f32, 1e30)
        if points:
            bufs["points"] = d.full((n, fh, fw, 16), np.uint8, SENTINEL)
        if compact:
            bufs["compact"] = d.full((n, fh, fw, 16), np.uint8, SENTINEL)
        if count or compact:
            bufs["count"] = d.full((n,), np.uint64, 12345)
        if want_mask:
            bufs["mask"] = d.full((n, 1, fh, fw), np.uint8, 7)
        if want_vcount:
            bufs["valid_count"] = d.full((n,), np.uint64, 12345)
        if "count" in bufs:
            bufs["ws"] = d.full((klib.points_workspace_bytes(n, fh, fw),), np.uint8, 0xEE)
    klib.disparity_to_points(d.put(px), n, h, w, fh, fw, cam, zmin, zmax, mask=None if mask is None else d.put(mask),
                             color=None if frames is None else d.put(frames), color_step=None if frames is None else frames.shape[2],
                             encoding=encoding, disp_out=bufs.get("disp"), disp_kind=PIXELS if disp_kind is None else disp_kind,
                             out_mask=bufs.get("mask"), valid_count=bufs.get("valid_count"), depth=bufs.get("depth"),
                             depth_kind=M_F32 if depth_kind is None else depth_kind, points=bufs.get("points"),
                             points_compact=bufs.get("compact"), count=bufs.get("count"), workspace=bufs.get("ws"), stream=stream)
    return read_points(d, bufs, disp_kind, depth_kind), bufs


def read_points(d, bufs, disp_kind, depth_kind):
    got = {}
    for key, b in bufs.items():
        if key == "ws" or b is None:
            continue
        if key == "disp":
            got[key] = d.get(b, np.uint16 if disp_kind == U16 else f32)
        elif key == "depth":
            got[key] = d.get(b, np.uint16) if depth_kind == MM_U16 else d.get(b, f32).view(u32)
        elif key in ("points", "compact"):
            got[key] = np.ascontiguousarray(d.get(b, np.uint8)).view(u32)
        elif key in ("count", "valid_count"):
            got[key] = d.get(b, np.uint64)
        else:
            got[key] = d.get(b, np.uint8)
    return got


def check_compact(got, ref, n, plane):
    """the compact cloud of a read-back against the restatement: the records, the count, the sentinel behind the last point"""
    assert np.array_equal(got["count"], ref["count"]), (got["count"], ref["count"])
    flat = got["compact"].reshape(n, plane, 4)
    for i in range(n):
        c = int(ref["count"][i])
        assert np.array_equal(flat[i, :c], ref["compact"][i]), (i, c)
        assert (flat[i, c:].view(np.uint8) == SENTINEL).all(), i


def assert_bits(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.dtype, ref.shape)
    assert np.array_equal(got, ref), (what, int((got != ref).sum()))


# ---- 1. bit for bit against the restatement -----------------------------------------------------------------------------------------------
SIZES = [((369, 1257), (375, 1242)), ((321, 1025), (376, 672)), ((25, 41), (25, 41)), ((25, 41), (19, 31))]
COLOURS = [(None, 0)] + [(e, p) for e in ENCODINGS for p in (0, PAD)]
VARIANTS = list(itertools.product((M_F32, MM_U16), (0.0, 3.25)))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("net,frame", SIZES, ids=["%dx%d-%dx%d" % (s[1], s[0], t[1], t[0]) for s, t in SIZES])
def test_bit_equal_to_restatement(backend, net, frame, masked):
    """batch 2 (odd planes: image 1 starts off a 16-byte boundary of the 4-byte outputs).  Without colour and with the left frame in all
    four encodings, dense and pitched; both depth kinds and doffs 0 / 3.25 take turns over the colour cases at the camera sizes and are
    all combined with every colour case at the small ones.  disp_out is rt_disparity_to_frame's output, of both kinds."""
    d = Bufs(backend.name == "gpu")
    k = backend.klib
    n, (fh, fw) = 2, frame
    px, mask = disparity_field(n, *net, seed=31, with_mask=masked)
    px = (px * f32(0.5)).astype(f32)
    if mask is not None:
        px[mask == 0] = 0
    bgr = images(n, fh, fw, seed=32)
    small = fh < 100
    for i, (enc, pad) in enumerate(COLOURS):
        for j, (depth_kind, doffs) in enumerate(VARIANTS if small else [VARIANTS[i % 4]]):
            cam = camera(fx=720.0 if small else 721.5377, fy=700.0 if small else 721.5377, cx=fw / 2 - 0.4407, cy=fh / 2 - 0.146, baseline=0.54,
                         doffs=doffs)
            zmin, zmax = (0.0, INF) if (i + j) % 3 == 0 else (5.0, 10.0)
            frames = None if enc is None else pack(bgr, enc, pad, seed=i)
            disp_kind = U16 if (i + j) % 2 else PIXELS
            ref = to_points(px, mask, fh, fw, cam, zmin, zmax, None if enc is None else rgb_of(bgr))
            got, _ = run_points(k, d, px, mask, fh, fw, cam, zmin, zmax, frames, enc if enc is not None else 0, disp_kind, depth_kind,
                                points=True, compact=True, want_mask=masked, want_vcount=masked)
            what = (enc, pad, depth_kind, doffs, zmin)
            assert_bits(got["depth"], ref["depth_mm"] if depth_kind == MM_U16 else ref["depth_m"], what)
            assert_bits(got["points"].reshape(n, fh, fw, 4), ref["points"], what)
            check_compact(got, ref, n, fh * fw)
            old = run_to_frame(backend, d, px, mask, fh, fw, disp_kind)
            assert_bits(got["disp"], old["out"], what)
            if masked:
                assert_bits(got["mask"], old["mask"], what)
                assert_bits(got["valid_count"], old["valid_count"], what)
            frac = ref["ok"].mean()
            assert 0.1 < frac <= 1.0 and (zmin == 0.0 or frac < 0.9), (what, frac)          # the range and the mask both bite
    # every output alone equals itself in company (one launch, uniform branches on the outputs present)
    cam = camera(cx=fw / 2, cy=fh / 2, baseline=0.54)
    ref = to_points(px, mask, fh, fw, cam, 0.0, INF, rgb_of(bgr))
    frames = pack(bgr, capi.RT_ENC_RGBA8, PAD, seed=5)
    for kw in (dict(depth_kind=M_F32), dict(depth_kind=MM_U16), dict(points=True), dict(count=True), dict(compact=True), dict(disp_kind=PIXELS)):
        got, _ = run_points(k, d, px, mask, fh, fw, cam, frames=frames, encoding=capi.RT_ENC_RGBA8, **kw)
        if "depth_kind" in kw:
            assert_bits(got["depth"], ref["depth_mm"] if kw["depth_kind"] == MM_U16 else ref["depth_m"], kw)
        if "points" in kw:
            assert_bits(got["points"].reshape(n, fh, fw, 4), ref["points"], kw)
        if "count" in kw:
            assert_bits(got["count"], ref["count"], kw)
        if "compact" in kw:
            check_compact(got, ref, n, fh * fw)
        if "disp_kind" in kw:
            assert_bits(got["disp"], to_frame(px, mask, fh, fw, PIXELS)["out"], kw)


# ---- 2. inputs that bite ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth_kind", [M_F32, MM_U16], ids=["metres", "millimetres"])
def test_special_inputs_follow_the_restatement(backend, depth_kind):
    """NaN, +-inf, negative and zero disparities; v + doffs exactly 0; Z exactly at min_depth and max_depth and one ulp outside;
    max_depth = +inf; Z * 1000 above 65535 and below 0.5 -- same size (the resampling is the identity) and resized, plain and masked"""
    d = Bufs(backend.name == "gpu")
    h, w = 25, 41
    cam = camera(fx=700.0, baseline=0.12, doffs=-2.0)
    fB = f32(f32(700.0) * f32(0.12))
    px, mask = disparity_field(2, h, w, seed=33, with_mask=True)
    mask[:, :, 2:9, 2:14] = 255
    row = px[0, 0, 4]
    with np.errstate(all="ignore"):
        zlo, zhi = f32(fB / f32(30.0)), f32(fB / f32(6.0))                       # Z of den = 30 and den = 6: the range used below
    row[2:14] = [np.nan, np.inf, -np.inf, -7.5, 0.0, 2.0, 32.0, 8.0, np.nextafter(f32(32.0), f32(100)), np.nextafter(f32(8.0), f32(0)), 1e30, 2.0 + 1e-3]
    px[1, 0, 5, 2:8] = [2.0 + 84.0 / 65.535, 2.0 + 84.0 / 70.0, 2.0 + 84.0 / 0.0004, 2.0 + 84.0 / 0.0006, 1e38, 3e38]
    assert f32(row[7] + f32(-2.0)) == 0 and f32(fB / f32(row[8] - 2)) == zlo and f32(fB / f32(row[9] - 2)) == zhi
    for m in (None, mask):
        for frame in ((h, w), (40, 66), (19, 31)):
            for zmin, zmax in ((0.0, INF), (float(zlo), float(zhi)), (0.0, 1e-3), (70.0, INF)):
                ref = to_points(px, m, *frame, cam, zmin, zmax)
                got, _ = run_points(backend.klib, d, px, m, *frame, cam, zmin, zmax, depth_kind=depth_kind, points=True, compact=True,
                                    disp_kind=PIXELS)
                what = (m is None, frame, zmin, zmax)
                assert_bits(got["depth"], ref["depth_mm"] if depth_kind == MM_U16 else ref["depth_m"], what)
                assert_bits(got["points"].reshape(2, *frame, 4), ref["points"], what)
                check_compact(got, ref, 2, frame[0] * frame[1])
                want = to_frame(px, m, *frame, PIXELS)["out"]
                assert np.array_equal(got["disp"], want, equal_nan=True), what      # the disparity follows its own validity, not the range
    # the restatement at the same size, where it can be read off by hand
    ref = to_points(px, None, h, w, cam, float(zlo), float(zhi))
    ok = ref["ok"][0, 4]
    assert list(ok[2:14]) == [False, False, False, False, False, False, True, True, False, False, False, False]
    assert ref["depth_m"][0, 0, 4, 8] == zlo.view(u32) and ref["depth_m"][0, 0, 4, 9] == zhi.view(u32) and ref["depth_m"][0, 0, 4, 2] == NAN_BITS
    ref = to_points(px, None, h, w, cam, 0.0, INF)
    assert list(ref["ok"][0, 4, 2:14]) == [False, False, False, False, False, False, True, True, True, True, True, True]
    assert ref["depth_mm"][0, 0, 4, 12] == 1 and ref["depth_mm"][0, 0, 4, 13] == 65535            # 8.4e-29 m -> 1 (not 0); 84 km saturates
    assert list(ref["depth_mm"][1, 0, 5, 2:6]) == [65535, 65535, 1, 1]                              # 65.535 m, 70 m, 0.4 mm, 0.6 mm


# ---- 3. compaction --------------------------------------------------------------------------------------------------------------------------
def test_compaction(backend):
    """The compact cloud is the organised cloud's ok records in row-major order and count their number; the bytes behind the last point
    of every image keep their sentinel, so images of a batch do not run into each other; an image with every point valid and one with
    none; two runs agree byte for byte.  On the GPU at 1242 x 375 (455 tiles an image), on the emulator also at a size of a few tiles."""
    d = Bufs(backend.name == "gpu")
    for (h, w), (fh, fw) in (((369, 1257), (375, 1242)), ((40, 66), (47, 80))):
        n = 4
        px, mask = disparity_field(n, h, w, seed=34, with_mask=True)
        px[2], mask[2] = 40.0, 255                                                  # every point valid
        mask[3] = 0                                                                 # none
        px[3] = 0
        bgr = images(n, fh, fw, seed=35)
        cam = camera(fx=721.5377, fy=721.5377, cx=fw / 2, cy=fh / 2, baseline=0.54)
        frames = pack(bgr, capi.RT_ENC_BGR8)
        ref = to_points(px, mask, fh, fw, cam, 2.0, 80.0, rgb_of(bgr))
        assert ref["count"][2] == fh * fw and ref["count"][3] == 0 and 0 < ref["count"][0] < fh * fw and ref["count"][0] != ref["count"][1]
        got, _ = run_points(backend.klib, d, px, mask, fh, fw, cam, 2.0, 80.0, frames, points=True, compact=True)
        org = got["points"].reshape(n, fh * fw, 4)
        assert_bits(org, ref["points"].reshape(n, fh * fw, 4))
        flat = got["compact"].reshape(n, fh * fw, 4)
        for i in range(n):
            c = int(got["count"][i])
            keep = org[i, :, 2] != NAN_BITS                                          # z is a number exactly where the point is ok
            assert c == keep.sum() == ref["count"][i], (i, c)
            assert np.array_equal(flat[i, :c], org[i][keep]), i
            assert (flat[i, c:].view(np.uint8) == SENTINEL).all(), i
        again, _ = run_points(backend.klib, d, px, mask, fh, fw, cam, 2.0, 80.0, frames, points=True, compact=True)
        for key in got:
            assert got[key].tobytes() == again[key].tobytes(), key
        # the count alone, and the compact cloud without the organised one
        alone, _ = run_points(backend.klib, d, px, mask, fh, fw, cam, 2.0, 80.0, frames, count=True)
        assert np.array_equal(alone["count"], ref["count"])
        only, _ = run_points(backend.klib, d, px, mask, fh, fw, cam, 2.0, 80.0, frames, compact=True)
        assert only["compact"].tobytes() == got["compact"].tobytes() and np.array_equal(only["count"], ref["count"])


# ---- 4. geometry against fp64 -----------------------------------------------------------------------------------------------------------------
def test_geometry_against_fp64(backend):
    """A fronto-parallel plane Z = 6 m and a slanted plane Z = 4 + 0.8 X + 0.3 Y, rendered exactly: with X = (u - cx) Z / fx and
    Y = (r - cy) Z / fy the slanted plane gives Z = 4 / (1 - 0.8 (u - cx) / fx - 0.3 (r - cy) / fy), and d = fx B / Z - doffs, in fp64.  The
    disparity is rounded to fp32 and fed at the same size, so the resampling is the identity (weights 1 and 0, the width ratio 1: exact).
    Reference: the three formulas evaluated in fp64 on the fp32 inputs (d, fx, fy, cx, cy, B, doffs as fp32 numbers).
    Bound.  Z = fB / (d + doffs) carries three roundings: the product fx * B, the sum, the division.  X and Y carry three more: the
    difference u - cx, the division by fx, the product with Z.  Each rounding contributes at most a relative 2^-24 to first order, so
    |Z - Z64| <= 3 * 2^-24 |Z| and |X - X64| <= 6 * 2^-24 |X|; the bound asked is 8 * 2^-24 relative for all three, which covers the
    second-order terms.  Where |u - cx| < 1 (|r - cy| < 1) the rounding of the difference is no longer small against the difference
    itself but is still at most 2^-25 in absolute terms (|u - cx| < 1), so there the bound is the absolute 8 * 2^-24 * Z / fx (Z / fy)."""
    d = Bufs(backend.name == "gpu")
    h, w = 120, 200
    cam = camera(fx=700.0, fy=705.5, cx=99.3, cy=60.2, baseline=0.12, doffs=1.75)
    fx, fy, cx, cy, B, doffs = (float(f32(x)) for x in (cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline, cam.doffs))
    u = np.arange(w, dtype=np.float64)[None, :]
    r = np.arange(h, dtype=np.float64)[:, None]
    planes = [np.full((h, w), 6.0), 4.0 / (1.0 - 0.8 * (u - cx) / fx - 0.3 * (r - cy) / fy)]
    px = np.stack([(fx * B / z - doffs).astype(f32) for z in planes])[:, None]
    assert px.min() > 5 and px.max() < 40
    got, _ = run_points(backend.klib, d, px, None, h, w, cam, points=True, depth_kind=M_F32)
    pts = got["points"].reshape(2, h, w, 4)[..., :3].copy().view(f32)
    assert np.array_equal(got["depth"][:, 0], got["points"].reshape(2, h, w, 4)[..., 2])
    d64 = px[:, 0].astype(np.float64)
    Z = fx * B / (d64 + doffs)
    X, Y = (u - cx) / fx * Z, (r - cy) / fy * Z
    eps = 8.0 * 2.0 ** -24
    for name, val, ref, near, scale in (("Z", pts[..., 2], Z, None, None), ("X", pts[..., 0], X, np.abs(u - cx) < 1, Z / fx),
                                        ("Y", pts[..., 1], Y, np.abs(r - cy) < 1, Z / fy)):
        err = np.abs(val.astype(np.float64) - ref)
        bound = eps * np.abs(ref)
        if near is not None:
            bound = np.where(np.broadcast_to(near, ref.shape), eps * scale, bound)
        worst = (err / bound).max()
        print("%s against fp64: worst error / bound = %.3f" % (name, worst))
        assert (err <= bound).all(), (name, worst)
    # the planes come back: the rendered disparity was rounded to fp32 (2^-24 relative, amplified by d / (d + doffs) < 1) on top of eps
    assert np.abs(pts[0, ..., 2] - 6.0).max() <= 6.0 * (eps + 2.0 ** -24)
    assert np.abs(pts[1, ..., 2] - (4.0 + 0.8 * pts[1, ..., 0] + 0.3 * pts[1, ..., 1])).max() <= 1e-5
    # one pixel by hand: fx = 700, B = 0.12, d = 42, doffs = 0 -> Z = 2, X = (u - cx) * 2 / 700
    cam = camera(fx=700.0, fy=700.0, cx=16.0, cy=8.0, baseline=0.12, doffs=0.0)
    px = np.full((1, 1, 20, 40), 42.0, f32)
    got, _ = run_points(backend.klib, d, px, None, 20, 40, cam, points=True)
    pts = got["points"].reshape(20, 40, 4)[..., :3].copy().view(f32)
    assert abs(pts[5, 30, 2] - 2.0) <= 2.0 * eps and abs(pts[5, 30, 0] - 14.0 * 2.0 / 700.0) <= eps * 0.04 and abs(pts[5, 30, 1] + 3.0 * 2.0 / 700.0) <= eps * 0.01
    assert pts[8, 16, 0] == 0 and pts[8, 16, 1] == 0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_op_refusals(backend):
    """every refusal of rt_disparity_to_points: an error (RT_E_UNSUPPORTED for the factors) and sentinel-filled outputs untouched"""
    d = Bufs(backend.name == "gpu")
    k = backend.klib
    px, mask = disparity_field(1, 10, 12, seed=36, with_mask=True)
    dpx, dm = d.put(px), d.put(mask)
    fh, fw = 70, 84
    bufs = dict(disp=d.nan(1, 1, fh, fw), mask=d.full((1, 1, fh, fw), np.uint8, 7), valid_count=d.full((1,), np.uint64, 12345),
                depth=d.full((1, 1, fh, fw), f32, 1e30), points=d.full((1, fh, fw, 16), np.uint8, SENTINEL),
                compact=d.full((1, fh, fw, 16), np.uint8, SENTINEL), count=d.full((1,), np.uint64, 12345),
                ws=d.full((k.points_workspace_bytes(1, fh, fw),), np.uint8, 0xEE))
    col = d.put(pack(images(1, fh, fw, 1), capi.RT_ENC_BGRA8))
    nan = float("nan")

    def call(disp_px=dpx, h=10, w=12, oh=20, ow=24, cam=None, batch=1, **kw):
        args = dict(mask=dm, color=col, color_step=4 * fw, encoding=capi.RT_ENC_BGRA8, disp_out=bufs["disp"], out_mask=bufs["mask"],
                    valid_count=bufs["valid_count"], depth=bufs["depth"], points=bufs["points"], points_compact=bufs["compact"],
                    count=bufs["count"], workspace=bufs["ws"])
        args.update(kw)
        k.disparity_to_points(disp_px, batch, h, w, oh, ow, camera() if cam is None else cam, **args)

    def untouched():
        g = {key: d.get(b, np.uint8 if key in ("mask", "points", "compact", "ws") else (np.uint64 if "count" in key else f32)) for key, b in bufs.items()}
        return (np.isnan(g["disp"]).all() and (g["mask"] == 7).all() and (g["valid_count"] == 12345).all() and (g["depth"] == f32(1e30)).all() and
                (g["points"] == SENTINEL).all() and (g["compact"] == SENTINEL).all() and (g["count"] == 12345).all() and (g["ws"] == 0xEE).all())

    none = dict(disp_out=None, out_mask=None, valid_count=None, depth=None, points=None, points_compact=None, count=None)
    cases = [
        dict(disp_px=None), dict(cam="null"), none,                                                       # null pointers, no output
        dict(batch=0), dict(h=0), dict(w=0), dict(oh=0), dict(ow=0),                                      # sizes < 1
        dict(cam=camera(fx=0.0)), dict(cam=camera(fx=-700.0)), dict(cam=camera(fx=nan)), dict(cam=camera(fx=INF)),
        dict(cam=camera(fy=0.0)), dict(cam=camera(fy=nan)), dict(cam=camera(fy=INF)),
        dict(cam=camera(baseline=0.0)), dict(cam=camera(baseline=-0.1)), dict(cam=camera(baseline=nan)), dict(cam=camera(baseline=INF)),
        dict(cam=camera(cx=nan)), dict(cam=camera(cx=INF)), dict(cam=camera(cy=nan)), dict(cam=camera(cy=-INF)),
        dict(cam=camera(doffs=nan)), dict(cam=camera(doffs=INF)),
        dict(min_depth=nan), dict(min_depth=-0.5), dict(max_depth=nan), dict(min_depth=2.0, max_depth=1.0), dict(min_depth=INF, max_depth=1.0),
        dict(disp_kind=capi.RT_DISP_NET), dict(disp_kind=3), dict(depth_kind=2), dict(depth_kind=-1),     # unknown kinds
        dict(encoding=4), dict(encoding=-1),                                                              # unknown encodings
        dict(color_step=4 * 24 - 1), dict(color_step=3 * 24 - 1, encoding=capi.RT_ENC_RGB8),              # a step shorter than a row
        dict(count=None),                                                                                 # points_compact without count
        dict(workspace=None), dict(workspace_bytes=k.points_workspace_bytes(1, 20, 24) - 1),              # no or a short workspace
        dict(points_compact=None, workspace=None),                                                        # ... for the count alone
        dict(mask=None),                                                                                  # mask outputs without a mask
    ]
    for i, kw in enumerate(cases):
        kw = dict(kw)
        if kw.get("cam") == "null":
            kw.pop("cam")
            with pytest.raises(capi.RtError):
                k.disparity_to_points(dpx, 1, 10, 12, 20, 24, None, depth=bufs["depth"])
        else:
            with pytest.raises(capi.RtError):
                call(**kw)
        assert untouched(), (i, kw)
    for kw in (dict(oh=71, ow=84), dict(oh=60, ow=85), dict(h=70, oh=10, ow=12), dict(w=84, oh=10, ow=12)):     # factors outside [1/6, 6]
        with pytest.raises(capi.RtError) as e:
            call(color=None, **kw)
        assert "(%d)" % -2 in str(e.value) and untouched(), (kw, str(e.value))                           # RT_E_UNSUPPORTED
    assert k.points_workspace_bytes(0, 20, 24) == 0 and k.points_workspace_bytes(1, 0, 24) == 0
    # ... and next to them it works: factor 6, max_depth = +inf, min_depth = max_depth
    call(oh=60, ow=72, color_step=4 * fw, min_depth=0.0, max_depth=INF)
    ref = to_points(px, mask, 60, 72, camera(), 0.0, INF)
    assert np.array_equal(d.get(bufs["count"], np.uint64), ref["count"]) and ref["count"][0] > 0
    call(oh=60, ow=72, min_depth=5.0, max_depth=5.0)
    assert np.array_equal(d.get(bufs["count"], np.uint64), to_points(px, mask, 60, 72, camera(), 5.0, 5.0)["count"])


# ---- 6. rt_net_execute_frames_3d on synthetic weights ------------------------------------------------------------------------------------------
def bufs_3d(d, n, sh, sw, disp, subset, check, depth_kind=M_F32, disp_kind=PIXELS):
    """sentinel-filled buffers of one call; subset: which of depth / points / compact are asked for"""
    b = dict(disp=None, mask=None, valid_count=None, depth=None, points=None, compact=None, count=None)
    if disp:
        b["disp"] = d.full((n, 1, sh, sw), np.uint16, 0xFFFF) if disp_kind == U16 else d.nan(n, 1, sh, sw)
        if check:
            b["mask"], b["valid_count"] = d.full((n, 1, sh, sw), np.uint8, 7), d.full((n,), np.uint64, 12345)
    if "depth" in subset:
        b["depth"] = d.full((n, 1, sh, sw), np.uint16, 0xFFFF) if depth_kind == MM_U16 else d.full((n, 1, sh, sw), f32, 1e30)
    if "points" in subset:
        b["points"] = d.full((n, sh, sw, 16), np.uint8, SENTINEL)
    if "compact" in subset:
        b["compact"], b["count"] = d.full((n, sh, sw, 16), np.uint8, SENTINEL), d.full((n,), np.uint64, 12345)
    return b


def call_3d(net, fl, fr, enc, cam, b, n, resize, max_diff, zmin=0.0, zmax=INF, depth_kind=M_F32, disp_kind=PIXELS, **kw):
    net.execute_frames_3d(fl, fr, enc, cam, disp=b["disp"], kind=disp_kind, resize=resize, max_diff_px=max_diff, mask=b["mask"],
                          valid_count=b["valid_count"], min_depth=zmin, max_depth=zmax, depth=b["depth"], depth_kind=depth_kind,
                          points=b["points"], points_compact=b["compact"], count=b["count"], batch=n, **kw)


def points_by_hand(lib, d, raw, n, h, w, scale, sh, sw, fl, step, enc, cam, max_diff, zmin, zmax, depth_kind, disp_kind):
    """the op-level calls a caller would write behind rt_net_execute: the definition of rt_net_execute_frames_3d (every output at once)"""
    k = lib.kernels
    check = max_diff >= 0
    mask = None
    if check:
        px, mask = d.nan(n, 1, h, w), d.full((n, 1, h, w), np.uint8, 7)
        k.lr_consistency(raw, n, h, w, float(scale), max_diff, px, PIXELS, mask, None, None)
    elif scale != 1:
        px = d.nan(n, 1, h, w)
        k.disparity_scale(raw, px, n * h * w, float(scale))
    else:
        px = raw
    b = bufs_3d(d, n, sh, sw, True, ("depth", "points", "compact"), check, depth_kind, disp_kind)
    ws = d.full((k.points_workspace_bytes(n, sh, sw),), np.uint8, 0)
    k.disparity_to_points(px, n, h, w, sh, sw, cam, zmin, zmax, mask=mask, color=fl, color_step=step, encoding=enc, disp_out=b["disp"],
                          disp_kind=disp_kind, out_mask=b["mask"], valid_count=b["valid_count"], depth=b["depth"], depth_kind=depth_kind,
                          points=b["points"], points_compact=b["compact"], count=b["count"], workspace=ws)
    return read_points(d, b, disp_kind, depth_kind)


def compare_3d(got, ref, n, plane, what):
    for key, v in got.items():
        if key == "compact":
            flat, want = v.reshape(n, plane, 4), ref["compact"].reshape(n, plane, 4)
            for i in range(n):
                c = int(ref["count"][i])
                assert np.array_equal(flat[i, :c], want[i, :c]) and (flat[i, c:].view(np.uint8) == SENTINEL).all(), (what, i)
        else:
            assert_bits(v, ref[key], (what, key))


SUBSETS = [s for r in range(4) for s in itertools.combinations(("depth", "points", "compact"), r)]


@pytest.mark.parametrize("model,flags", NETS, ids=NET_IDS)
def test_execute_frames_3d_equals_the_pipeline_by_hand(rt, model, flags):
    """Every subset of the three 3-D outputs with call->disp given and NULL (15 calls; the empty subset needs a disparity), the four
    combinations of check x resize mode taking turns over them (frames 36 x 30 for RT_RESIZE_CV_AREA: x grows, y shrinks; 83 x 51 for
    RT_RESIZE_AREA_DOWN), both depth and disparity kinds alternating: each output bit-equal to the op-level calls made by hand.
    out == NULL is rt_net_execute_frames_ex; RT_GEOM_NET and the refusals of either struct write nothing."""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    net, h, w, scale = make_net(lib, model, flags)
    n, enc = (2 if flags else 1), capi.RT_ENC_BGRA8
    modes = [(CV, -1.0, 30, 36), (DOWN, 1.5, 51, 83), (CV, 1.5, 30, 36), (DOWN, -1.0, 51, 83)]
    frames, raws, refs = {}, {}, {}
    for sh, sw in ((30, 36), (51, 83)):
        frames[sh] = (d.put(pack(images(n, sh, sw, 21), enc, PAD, 11)), d.put(pack(images(n, sh, sw, 22), enc, PAD, 12)))
    calls = [(disp, s) for disp in (True, False) for s in SUBSETS if disp or s]
    assert len(calls) == 15
    for i, (disp, subset) in enumerate(calls):
        resize, max_diff, sh, sw = modes[i % 4]
        depth_kind, disp_kind = (M_F32, MM_U16)[(i // 4) % 2], (PIXELS, U16)[(i // 2) % 2]
        zmin, zmax = ((0.0, INF), (0.05, 1.0))[i % 2]
        cam = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)
        fl, fr = frames[sh]
        step, check = fl.shape[2], max_diff >= 0
        if (resize, check) not in raws:
            il, ir, raw = d.nan(2 * n, 3, h, w), d.nan(2 * n, 3, h, w), d.nan(2 * n, 1, h, w)
            m = 2 * n if check else n
            if resize == CV:
                lib.kernels.preprocess_frames_u8_cv(fl, fr, sh, sw, step, enc, il, ir, h, w, n, mirror_twin=check)
            else:
                (lib.kernels.preprocess_frames_u8_lr if check else lib.kernels.preprocess_frames_u8)(fl, fr, sh, sw, step, enc, il, ir, h, w, n)
            net.execute(il, ir, raw, m)
            raws[(resize, check)] = raw
        key = (resize, check, depth_kind, disp_kind, zmin)
        if key not in refs:
            refs[key] = points_by_hand(lib, d, raws[(resize, check)], n, h, w, scale, sh, sw, fl, step, enc, cam, max_diff, zmin, zmax,
                                       depth_kind, disp_kind)
            print("ok fraction", key, refs[key]["count"].sum() / (n * sh * sw))
        b = bufs_3d(d, n, sh, sw, disp, subset, check, depth_kind, disp_kind)
        call_3d(net, fl, fr, enc, cam, b, n, resize, max_diff, zmin, zmax, depth_kind, disp_kind, src_w=sw)
        compare_3d(read_points(d, b, disp_kind, depth_kind), refs[key], n, sh * sw, (i, disp, subset, key))
    # out == NULL: rt_net_execute_frames_ex
    sh, sw = 30, 36
    fl, fr = frames[sh]
    for max_diff in (-1.0, 1.5):
        old = read(d, call_ex(d, net, fl, fr, enc, n, sh, sw, PIXELS, G_FRAME, CV, max_diff, src_w=sw), PIXELS)
        new = outputs(d, n, sh, sw, PIXELS)
        check = max_diff >= 0
        net.execute_frames_3d(fl, fr, enc, None, disp=new["out"], resize=CV, max_diff_px=max_diff, mask=new["mask"] if check else None,
                              valid_count=new["valid_count"] if check else None, batch=n, src_w=sw, no_depth_call=True)
        new = read(d, new, PIXELS)
        for key in old:
            assert np.array_equal(new[key], old[key]), (max_diff, key)
    # refusals: RT_GEOM_NET with a message that says so, either struct's size, the op's own arguments -- nothing written
    cam = camera(fx=30.0, fy=31.0, cx=18.0, cy=15.0, baseline=0.1)
    b = bufs_3d(d, n, sh, sw, True, ("depth", "points", "compact"), True)
    nan = float("nan")

    def untouched():
        g = read_points(d, b, PIXELS, M_F32)
        return (np.isnan(g["disp"]).all() and (g["mask"] == 7).all() and (g["valid_count"] == 12345).all() and
                (g["depth"] == f32(1e30).view(u32)).all() and (g["points"].view(np.uint8) == SENTINEL).all() and
                (g["compact"].view(np.uint8) == SENTINEL).all() and (g["count"] == 12345).all())

    with pytest.raises(capi.RtError) as e:
        call_3d(net, fl, fr, enc, cam, b, n, CV, 1.5, src_w=sw, geometry=G_NET)
    assert "RT_GEOM_NET" in str(e.value) and "(%d)" % -2 in str(e.value) and untouched(), str(e.value)
    big_l, big_r = d.put(pack(images(5, sh, sw, 1), enc)), d.put(pack(images(5, sh, sw, 2), enc))
    small = d.put(pack(images(n, 20, 30, 3), enc))          # the down-only filter refuses it: both axes would grow
    bad = [dict(struct_bytes=ctypes.sizeof(capi.FrameCall) - 8), dict(depth_struct_bytes=ctypes.sizeof(capi.DepthCall) - 8), dict(depth_struct_bytes=0),
           dict(resize=2), dict(geometry=2), dict(disp_kind=3), dict(disp_kind=capi.RT_DISP_NET), dict(depth_kind=2), dict(max_diff=nan),
           dict(cam=camera(fx=0.0)), dict(cam=camera(fy=nan)), dict(cam=camera(baseline=-1.0)), dict(cam=camera(cx=INF)), dict(cam=camera(cy=nan)),
           dict(cam=camera(doffs=nan)), dict(zmin=-1.0), dict(zmin=nan), dict(zmax=nan), dict(zmin=2.0, zmax=1.0), dict(enc=9),
           dict(batch=3, fl=big_l, fr=big_r), dict(batch=0), dict(resize=DOWN, fl=small, fr=small), dict(src_step=4 * sw - 1)]
    for kw in bad:
        kw = dict(kw)
        args = dict(resize=CV, max_diff=1.5, cam=cam, enc=enc, fl=fl, fr=fr, batch=n)
        for key in list(args):
            if key in kw:
                args[key] = kw.pop(key)
        with pytest.raises(capi.RtError):
            call_3d(net, args["fl"], args["fr"], args["enc"], args["cam"], b, args["batch"], args["resize"], args["max_diff"],
                    src_w=30 if args["fl"] is small else sw, **kw)
        assert untouched(), kw
    for kw in (dict(compact=b["compact"], count=None), dict(mask=b["mask"], max_diff=-1.0), dict()):        # compact without count; a mask without
        bb = dict(b)                                                                                    # a check; nothing asked for at all
        bb.update({key: v for key, v in kw.items() if key != "max_diff"})
        if not kw:
            bb = dict.fromkeys(b)
        with pytest.raises(capi.RtError):
            call_3d(net, fl, fr, enc, cam, bb, n, CV, kw.get("max_diff", 1.5), src_w=sw)
        assert untouched(), kw
    net.destroy()


# ---- 7. GPU only: the reference's sample pair and trained weights; graph mode ---------------------------------------------------------------------
KITTI = dict(fx=721.5377, fy=721.5377, cx=609.5593, cy=172.854, baseline=0.54)


@pytest.mark.gpu
def test_reference_sample_pair_depth_and_cloud():
    """the reference's 1242 x 375 pair through ResNet-18 2D 1257 x 369 fp32 with a KITTI calibration and a check at 1 px: depth is finite
    and positive wherever the mask is valid, the cloud's z is the depth image bit for bit, count is the number of finite depths, the
    cloud's colour is the left frame, and everything equals the pipeline by hand"""
    lib, d = netlib("gpu"), Bufs(True)
    w, h = 1257, 369
    net = lib.create("resnet18_2D", w, h, max_batch=2, weights_path=model_files.weight_file("resnet18_2D"))
    left, right = sample_bgr()
    sh, sw = left.shape[1:3]
    assert (sh, sw) == (375, 1242)
    enc = capi.RT_ENC_BGR8
    fl, fr = d.put(pack(left, enc)), d.put(pack(right, enc))
    cam = camera(**KITTI)
    b = bufs_3d(d, 1, sh, sw, True, ("depth", "points", "compact"), True)
    call_3d(net, fl, fr, enc, cam, b, 1, CV, 1.0, src_w=sw)
    got = read_points(d, b, PIXELS, M_F32)
    depth = got["depth"].view(f32)[0, 0]
    valid = got["mask"][0, 0] != 0
    assert 0 < valid.sum() < sh * sw
    assert np.isfinite(depth[valid]).all() and (depth[valid] > 0).all() and np.isnan(depth[~valid]).all()
    pts = got["points"].reshape(sh, sw, 4)
    assert np.array_equal(pts[..., 2], got["depth"][0, 0])
    assert np.array_equal(pts[..., 3], rgb_of(left)[0])
    assert got["count"][0] == np.isfinite(depth).sum() == got["valid_count"][0]
    print("sample pair: %.1f %% of the frame has a depth, median %.2f m, range %.2f .. %.2f m"
          % (100.0 * valid.mean(), np.median(depth[valid]), depth[valid].min(), depth[valid].max()))
    raw = engine_by_hand(lib, d, net, fl, fr, sh, sw, 3 * sw, enc, h, w, 1, True)
    ref = points_by_hand(lib, d, raw, 1, h, w, w, sh, sw, fl, 3 * sw, enc, cam, 1.0, 0.0, INF, M_F32, PIXELS)
    compare_3d(got, ref, 1, sh * sw, "sample pair")
    # a depth range, millimetres, no check: count follows the range
    b = bufs_3d(d, 1, sh, sw, False, ("depth", "compact"), False, MM_U16)
    call_3d(net, fl, fr, enc, cam, b, 1, CV, -1.0, 5.0, 30.0, MM_U16, src_w=sw)
    got = read_points(d, b, PIXELS, MM_U16)
    mm = got["depth"][0, 0]
    assert got["count"][0] == (mm != 0).sum() and 0 < got["count"][0] < sh * sw and mm[mm != 0].min() >= 5000 and mm.max() <= 30000
    net.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("streams", [2, 1])
def test_graph_mode_with_rotating_buffers_depth_and_cloud(streams):
    """a camera ring: three sets of frame, disparity, depth and cloud buffers in rotation, on a torch stream and on the NULL stream, graph
    mode on, with a check -- every rotation bit-equal to the non-graph result"""
    lib, d = netlib("gpu"), Bufs(True)
    h, w, n, sh, sw = 129, 257, 2, 120, 300                  # x shrinks, y grows
    net = lib.create("resnet18_2D", w, h, max_batch=2 * n, weights=O.synth_weights_resnet18_2d(), max_disp=16)
    net.set_streams(streams)
    enc = capi.RT_ENC_BGRA8
    cam = camera(fx=300.0, fy=300.0, cx=150.2, cy=59.7, baseline=0.2)
    sets = [(d.put(pack(images(n, sh, sw, 40 + 2 * i), enc, PAD, i)), d.put(pack(images(n, sh, sw, 41 + 2 * i), enc, PAD, i + 7))) for i in range(3)]
    subset = ("depth", "points", "compact")

    def run(i, b, stream=None):
        call_3d(net, sets[i][0], sets[i][1], enc, cam, b, n, CV, 1.0, 0.5, 60.0, src_w=sw, stream=stream)

    direct = []
    for i in range(3):
        b = bufs_3d(d, n, sh, sw, True, subset, True)
        run(i, b)
        direct.append(read_points(d, b, PIXELS, M_F32))
    assert 0 < direct[0]["count"].sum() < n * sh * sw and direct[0]["points"].tobytes() != direct[1]["points"].tobytes()
    raw = engine_by_hand(lib, d, net, sets[0][0], sets[0][1], sh, sw, sets[0][0].shape[2], enc, h, w, n, True)
    ref = points_by_hand(lib, d, raw, n, h, w, w, sh, sw, sets[0][0], sets[0][0].shape[2], enc, cam, 1.0, 0.5, 60.0, M_F32, PIXELS)
    compare_3d(direct[0], ref, n, sh * sw, "direct")
    net.set_graph(True)
    s = torch.cuda.Stream()
    for call in range(9):                                 # 1: direct, 2: capture + launch, then replays, whatever pointers rotate in
        i = call % 3
        b = bufs_3d(d, n, sh, sw, True, subset, True)      # fresh sentinel-filled buffers: other pointers on every call
        torch.cuda.synchronize()
        run(i, b, stream=s.cuda_stream)
        s.synchronize()
        got = read_points(d, b, PIXELS, M_F32)
        for key in got:
            assert got[key].tobytes() == direct[i][key].tobytes(), (call, key)
    ring = [bufs_3d(d, n, sh, sw, True, subset, True) for _ in range(3)]
    for call in range(6):
        i = (call + 1) % 3
        ring[i]["depth"].fill_(1e30)
        ring[i]["compact"].fill_(SENTINEL)
        torch.cuda.synchronize()
        run(i, ring[i])
        got = read_points(d, ring[i], PIXELS, M_F32)
        for key in got:
            assert got[key].tobytes() == direct[i][key].tobytes(), (call, key)
    net.destroy()
