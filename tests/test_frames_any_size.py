"""Frames of any size in, disparity at the frame's size out.

- rt_preprocess_frames_u8_cv: the whole of cv::resize(INTER_AREA) as the ROS node calls it (reference stereo_dnn_ros_node.cpp:42-58).
  When neither axis grows it is rt_preprocess_frames_u8 (bit-identical); when either axis grows, OpenCV takes the two-tap set-up of its
  area_mode branch on BOTH axes.  `cv_area_taps` / `resize_cv_area_grow` below restate that in numpy (positions in double, weights and
  values in float32, every operation rounded on its own); the kernel must equal them bit for bit.  OpenCV itself is not available to
  these tests, so the restatement is held by properties instead: integer magnification replicates pixels, a constant stays constant,
  and on the reference's sample frame it stays within 1e-2 (max) / 1e-4 (mean) of the oracle's overlap-integral area filter.
- rt_disparity_to_frame: network-geometry pixels (+ the mask of rt_lr_consistency) -> the frame's geometry and pixels; `to_frame`
  restates it in numpy float32, bit for bit; a looser second check against torch's bilinear interpolation on a smooth map.
- rt_net_execute_frames_ex: the two around one engine pass (+ rt_lr_consistency), bit-equal to the op-level calls made by hand, and to
  rt_net_execute_frames / _lr where it is asked for what they do.
CPU tier: the same sources on the SIMT emulator; GPU tier (-m gpu): the MI355X, the reference's sample pair and trained weights."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import stereo_oracle as O
from redtail_amd import capi, model_files
from test_camera_frames import ENCODINGS, PAD, PAD_BYTE, images, netlib, pack, rt, sample_bgr  # noqa: F401  (rt: the emu / gpu fixture)
from test_lr_consistency import Bufs, make_net

f32 = np.float32
NET, PIXELS, U16 = capi.RT_DISP_NET, capi.RT_DISP_PIXELS_F32, capi.RT_DISP_KITTI_U16
CV, DOWN = capi.RT_RESIZE_CV_AREA, capi.RT_RESIZE_AREA_DOWN
G_NET, G_FRAME = capi.RT_GEOM_NET, capi.RT_GEOM_FRAME


# ---- the definitions restated in numpy --------------------------------------------------------------------------------------------------
def cv_area_taps(n, m):
    """front end, one axis, either axis grows: source n -> destination m"""
    inv = float(m) / float(n)
    scale = 1.0 / inv
    s0 = np.zeros(m, np.int64); s1 = np.zeros(m, np.int64); w1 = np.zeros(m, f32)
    for d in range(m):
        s = int(np.floor(d * scale))
        f = f32((d + 1) - (s + 1) * inv)
        f = f32(0) if f <= 0 else f32(f - f32(np.floor(f)))
        if s >= n - 1:
            s, f = n - 1, f32(0)
        s0[d], s1[d], w1[d] = s, min(s + 1, n - 1), f
    return s0, s1, (f32(1) - w1).astype(f32), w1


def resize_cv_area_grow(x, dh, dw):
    """x: (H, W, C) float32 holding the u8 values, memory channel order"""
    x0, x1, a0, a1 = cv_area_taps(x.shape[1], dw)
    y0, y1, b0, b1 = cv_area_taps(x.shape[0], dh)
    rows = (x[:, x0] * a0[None, :, None]).astype(f32) + (x[:, x1] * a1[None, :, None]).astype(f32)
    return ((rows[y0] * b0[:, None, None]).astype(f32) + (rows[y1] * b1[:, None, None]).astype(f32)).astype(f32)


def cv_planes(bgr, dh, dw):
    """(N,H,W,3) BGR uint8 -> (N,3,dh,dw) float32 RGB planes in [0,1]: what rt_preprocess_frames_u8_cv writes when an axis grows"""
    assert dh > bgr.shape[1] or dw > bgr.shape[2]
    return np.stack([(resize_cv_area_grow(img.astype(f32), dh, dw)[:, :, ::-1].transpose(2, 0, 1) / f32(255)).astype(f32) for img in bgr])


def with_twin(left, right):
    """the 2N images of a side with mirror_twin: [N, 2N) of the left side are the mirrored right planes and the other way round"""
    return np.concatenate([left, right[..., ::-1]]), np.concatenate([right, left[..., ::-1]])


def frame_taps(n, m):
    """back end, one axis: network n -> frame m"""
    sc = f32(n) / f32(m)
    d = np.arange(m, dtype=f32)
    p = np.maximum(((d + f32(0.5)) * sc).astype(f32) - f32(0.5), f32(0)).astype(f32)
    i0 = np.minimum(np.floor(p).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    w1 = (p - i0.astype(f32)).astype(f32)
    return i0, i1, (f32(1) - w1).astype(f32), w1


def encode_u16(v):
    """rintf(v * 256.f) saturated to [0, 65535]; a NaN encodes to 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(v * f32(256))
        q = np.where(q > 0, np.minimum(q, f32(65535)), f32(0))
    return q.astype(np.uint16)


def to_frame(px, mask, fh, fw, kind):
    """what rt_disparity_to_frame must write, bit for bit.  px: (N,1,H,W) float32, mask: (N,1,H,W) uint8 or None.
    Returns dict(out=, mask=, valid_count=) (the last two only with a mask)."""
    px = np.asarray(px, f32)[:, 0]
    _, H, W = px.shape
    r = f32(fw) / f32(W)
    y0, y1, b0, b1 = frame_taps(H, fh)
    x0, x1, a0, a1 = frame_taps(W, fw)

    def at(a, yy, xx):
        return a[:, yy][:, :, xx]

    with np.errstate(invalid="ignore", over="ignore"):
        top = (at(px, y0, x0) * a0[None, None]).astype(f32) + (at(px, y0, x1) * a1[None, None]).astype(f32)
        bot = (at(px, y1, x0) * a0[None, None]).astype(f32) + (at(px, y1, x1) * a1[None, None]).astype(f32)
        v = (((top * b0[None, :, None]).astype(f32) + (bot * b1[None, :, None]).astype(f32)).astype(f32) * r).astype(f32)
        valid = None
        if mask is not None:
            m = np.asarray(mask)[:, 0] != 0
            ny, nx = np.where(b1 > f32(0.5), y1, y0), np.where(a1 > f32(0.5), x1, x0)
            all4 = at(m, y0, x0) & at(m, y0, x1) & at(m, y1, x0) & at(m, y1, x1)
            v = np.where(all4, v, (at(px, ny, nx) * r).astype(f32))
            valid = at(m, ny, nx)
    if kind == U16:
        enc = encode_u16(v)
        if valid is not None:
            enc = np.maximum(enc, 1)                      # a valid 0 is raised to 1
    else:
        enc = v
    if valid is None:
        return dict(out=np.ascontiguousarray(enc)[:, None])
    return dict(out=np.where(valid, enc, enc.dtype.type(0))[:, None], mask=(valid * np.uint8(255))[:, None],
                valid_count=valid.sum(axis=(1, 2)).astype(np.uint64))


def test_restatements_have_the_properties_the_definitions_promise():
    """CPU only, no library: weights in [0, 1), first taps non-decreasing, every source pixel used, integer factors replicate"""
    for n, m in ((1242, 1257), (375, 369), (672, 1025), (376, 321), (70, 80), (59, 60), (37, 74), (59, 177)):
        s0, s1, w0, w1 = cv_area_taps(n, m)
        assert (w1 >= 0).all() and (w1 < 1).all() and (np.diff(s0) >= 0).all() and s0.min() == 0 and s1.max() == n - 1
        assert set(range(n)) <= set(s0[w0 > 0]) | set(s1[w1 > 0]), (n, m)
    x = images(1, 37, 59, 1)[0].astype(f32)
    assert np.array_equal(resize_cv_area_grow(x, 74, 118), np.repeat(np.repeat(x, 2, 0), 2, 1))
    assert np.array_equal(resize_cv_area_grow(x, 37, 177), np.repeat(x, 3, 1))


# ---- 1. front end, an axis grows ------------------------------------------------------------------------------------------------------
GROW_SIZES = [((375, 1242), (369, 1257)), ((376, 672), (321, 1025)), ((37, 59), (74, 118)), ((37, 59), (37, 177)), ((40, 66), (47, 80)),
              ((20, 30), (25, 41))]


@pytest.mark.parametrize("pad", [0, PAD], ids=["dense", "pitched"])
@pytest.mark.parametrize("encoding", ENCODINGS, ids=["bgr8", "rgb8", "bgra8", "rgba8"])
@pytest.mark.parametrize("src,dst", GROW_SIZES, ids=["%dx%d-%dx%d" % (s[1], s[0], t[1], t[0]) for s, t in GROW_SIZES])
def test_front_end_grow_bit_equal_to_restatement(backend, src, dst, encoding, pad):
    """batch 2 with different left / right content, mirror_twin 0 and 1, outputs pre-filled with NaN"""
    d = Bufs(backend.name == "gpu")
    n = 2
    left, right = images(n, *src, seed=3), images(n, *src, seed=4)
    fl, fr = pack(left, encoding, pad, 1), pack(right, encoding, pad, 2)
    step = fl.shape[2]
    ref_l, ref_r = cv_planes(left, *dst), cv_planes(right, *dst)
    if (dst[0] % src[0], dst[1] % src[1]) == (0, 0):             # integer factors: INTER_AREA replicates pixels
        ky, kx = dst[0] // src[0], dst[1] // src[1]
        rep = np.repeat(np.repeat(left[..., ::-1].transpose(0, 3, 1, 2).astype(f32), ky, 2), kx, 3) / f32(255)
        assert np.array_equal(ref_l, rep)
    for twin in (0, 1):
        m = 2 * n if twin else n
        ol, orr = d.nan(m, 3, *dst), d.nan(m, 3, *dst)
        backend.klib.preprocess_frames_u8_cv(d.put(fl), d.put(fr), src[0], src[1], step, encoding, ol, orr, dst[0], dst[1], n, mirror_twin=twin)
        want_l, want_r = with_twin(ref_l, ref_r) if twin else (ref_l, ref_r)
        got_l, got_r = d.get(ol), d.get(orr)
        assert np.array_equal(got_l, want_l), (twin, int((got_l != want_l).sum()))
        assert np.array_equal(got_r, want_r), (twin, int((got_r != want_r).sum()))
    if pad:                                                          # padding bytes are never read into the result
        fl2 = fl.copy()
        fl2[:, :, step - pad:] ^= 0x5C
        ol2, orr2 = d.nan(n, 3, *dst), d.nan(n, 3, *dst)
        backend.klib.preprocess_frames_u8_cv(d.put(fl2), d.put(fr), src[0], src[1], step, encoding, ol2, orr2, dst[0], dst[1], n)
        assert np.array_equal(d.get(ol2), ref_l)


def test_front_end_grow_properties(backend):
    """a constant frame stays that constant; on the reference's sample frame 1242 x 375 -> 1257 x 369 the result stays close to the
    oracle's overlap-integral area filter (a different, equally legitimate area filter, pinned to the reference's .bin)"""
    d = Bufs(backend.name == "gpu")
    k = backend.klib
    for value in (0, 1, 77, 200, 255):
        img = np.full((1, 40, 66, 3), value, np.uint8)
        src = d.put(pack(img, capi.RT_ENC_BGR8))
        ol, orr = d.nan(1, 3, 47, 80), d.nan(1, 3, 47, 80)
        k.preprocess_frames_u8_cv(src, src, 40, 66, 198, capi.RT_ENC_BGR8, ol, orr, 47, 80, 1)
        err = np.abs(d.get(ol).astype(np.float64) - value / 255.0).max()
        assert err <= 1e-6, (value, err)
    left = sample_bgr()[0]
    assert left.shape == (1, 375, 1242, 3)
    src = d.put(pack(left, capi.RT_ENC_BGR8))
    ol, orr = d.nan(1, 3, 369, 1257), d.nan(1, 3, 369, 1257)
    k.preprocess_frames_u8_cv(src, src, 375, 1242, 3 * 1242, capi.RT_ENC_BGR8, ol, orr, 369, 1257, 1)
    got = d.get(ol)[0]
    assert np.array_equal(got, d.get(orr)[0]) and np.array_equal(got, cv_planes(left, 369, 1257)[0])
    area = O.resize_area_tf(left[0].astype(f32), 369, 1257)[:, :, ::-1].transpose(2, 0, 1) / 255.0
    diff = np.abs(got.astype(np.float64) - area)
    print("cv two-tap vs overlap-integral area filter on the sample frame, / 255: mean %.3g max %.3g; image mean %.6f vs source %.6f"
          % (diff.mean(), diff.max(), got.mean(dtype=np.float64), left.mean(dtype=np.float64) / 255))
    assert diff.mean() <= 1e-4 and diff.max() <= 1e-2, (diff.mean(), diff.max())


# ---- 2. front end, shrinking or same size: the existing kernels -------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", [capi.RT_ENC_BGR8, capi.RT_ENC_RGBA8], ids=["bgr8", "rgba8"])
@pytest.mark.parametrize("src,dst", [((37, 59), (37, 59)), ((375, 1242), (321, 1025)), ((40, 66), (20, 33)), ((50, 97), (9, 17))])
def test_front_end_box_case_is_the_existing_entry(backend, src, dst, encoding):
    d = Bufs(backend.name == "gpu")
    n = 2
    fl, fr = pack(images(n, *src, seed=5), encoding, PAD, 1), pack(images(n, *src, seed=6), encoding, PAD, 2)
    step = fl.shape[2]
    for twin in (0, 1):
        m = 2 * n if twin else n
        ol, orr, rl, rr = (d.nan(m, 3, *dst) for _ in range(4))
        backend.klib.preprocess_frames_u8_cv(d.put(fl), d.put(fr), src[0], src[1], step, encoding, ol, orr, dst[0], dst[1], n, mirror_twin=twin)
        old = backend.klib.preprocess_frames_u8_lr if twin else backend.klib.preprocess_frames_u8
        old(d.put(fl), d.put(fr), src[0], src[1], step, encoding, rl, rr, dst[0], dst[1], n)
        assert np.array_equal(d.get(ol), d.get(rl)) and np.array_equal(d.get(orr), d.get(rr)), twin          # (NaN-free: array_equal)


# ---- 3. back end ------------------------------------------------------------------------------------------------------------------------
def disparity_field(n, h, w, seed, with_mask):
    """random disparities 0 .. 190 px with a few tiny ones (16-bit code 0); mask: ~10 % random zeros and a solid invalid band, the
    disparity 0 where the mask is 0, as rt_lr_consistency leaves it"""
    rng = np.random.default_rng(seed)
    px = rng.uniform(0, 190, (n, 1, h, w)).astype(f32)
    px[rng.uniform(size=px.shape) < 0.02] = f32(1e-3)
    if not with_mask:
        return px, None
    mask = np.where(rng.uniform(size=px.shape) < 0.1, 0, 255).astype(np.uint8)
    mask[:, :, h // 3:h // 3 + max(2, h // 8), w // 4:w // 4 + max(3, w // 5)] = 0
    px[mask == 0] = 0
    return px, mask


def run_to_frame(backend, d, px, mask, oh, ow, kind, want_mask=True, want_count=True):
    n, _, h, w = px.shape
    out = d.full((n, 1, oh, ow), np.uint16, 0xFFFF) if kind == U16 else d.nan(n, 1, oh, ow)
    om = d.full((n, 1, oh, ow), np.uint8, 7) if mask is not None and want_mask else None
    cnt = d.full((n,), np.uint64, 12345) if mask is not None and want_count else None
    backend.klib.disparity_to_frame(d.put(px), n, h, w, out, oh, ow, kind=kind, mask=None if mask is None else d.put(mask), out_mask=om,
                                    valid_count=cnt)
    got = dict(out=d.get(out, np.uint16 if kind == U16 else f32))
    if om is not None:
        got["mask"] = d.get(om, np.uint8)
    if cnt is not None:
        got["valid_count"] = d.get(cnt, np.uint64)
    return got


def assert_same(got, ref, what=""):
    for key, v in got.items():
        assert v.dtype == ref[key].dtype and v.shape == ref[key].shape, (what, key, v.dtype, v.shape, ref[key].dtype, ref[key].shape)
        assert np.array_equal(v, ref[key]), (what, key, int((v != ref[key]).sum()))


BACK_SIZES = [((369, 1257), (375, 1242)), ((321, 1025), (376, 672)), ((257, 513), (375, 1242)), ((25, 41), (20, 30)), ((25, 41), (25, 41))]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("kind", [PIXELS, U16], ids=["pixels", "kitti-u16"])
@pytest.mark.parametrize("net,frame", BACK_SIZES, ids=["%dx%d-%dx%d" % (s[1], s[0], t[1], t[0]) for s, t in BACK_SIZES])
def test_back_end_bit_equal_to_restatement(backend, net, frame, kind, masked):
    d = Bufs(backend.name == "gpu")
    n = 3                                                 # odd plane sizes: images 1 and 2 start off a 16-byte boundary
    px, mask = disparity_field(n, *net, seed=11, with_mask=masked)
    ref = to_frame(px, mask, *frame, kind)
    got = run_to_frame(backend, d, px, mask, *frame, kind)
    assert_same(got, ref)
    if masked:
        assert np.array_equal(got["valid_count"], (got["mask"] != 0).sum(axis=(1, 2, 3)).astype(np.uint64))
        assert (got["out"][got["mask"] == 0] == 0).all()
        frac = (got["mask"] != 0).mean()
        assert 0.5 < frac < 0.95, frac
        if kind == U16:
            assert (got["out"][got["mask"] != 0] >= 1).all()
            assert net[0] < 100 or (got["out"][got["mask"] != 0] == 1).any()                                   # a valid 0 became 1
        # the optional outputs may be absent
        assert_same(run_to_frame(backend, d, px, mask, *frame, kind, want_mask=False, want_count=False), dict(out=ref["out"]))
    if frame == net and not masked:                       # same size: a copy / the encoding of rt_disparity_to_u16
        assert np.array_equal(got["out"], px if kind == PIXELS else O.disparity_to_u16(px, 256.0))


@pytest.mark.parametrize("kind", [PIXELS, U16], ids=["pixels", "kitti-u16"])
def test_back_end_nan_negative_and_large_inputs_follow_the_restatement(backend, kind):
    d = Bufs(backend.name == "gpu")
    px, mask = disparity_field(2, 25, 41, seed=12, with_mask=True)
    px[0, 0, 5, 7], px[0, 0, 12, 30], px[1, 0, 3, 3] = np.nan, -3.5, 400.0
    px[1, 0, 20, 10:14] = [-0.25, 1e30, np.inf, -np.inf]
    mask[0, 0, 4:7, 6:9] = 255
    mask[1, 0, 19:22, 9:15] = 255
    for m in (None, mask):
        for frame in ((20, 30), (60, 97), (25, 41)):
            ref = to_frame(px, m, *frame, kind)
            got = run_to_frame(backend, d, px, m, *frame, kind)
            for key in got:
                assert got[key].dtype == ref[key].dtype
                assert np.array_equal(got[key], ref[key], equal_nan=(key == "out" and kind == PIXELS)), (key, frame, m is None)
            if kind == PIXELS:
                assert np.isnan(ref["out"]).any() and np.array_equal(np.isnan(got["out"]), np.isnan(ref["out"]))


def test_back_end_against_torch_bilinear():
    """the restatement (which the kernel equals bit for bit) against torch's CPU bilinear on a smooth map: a 0-190 px ramp plus a
    low-frequency wave.  The two differ by the fp32 rounding of the source coordinate times the map's gradient only; bound: 1e-3 px, a
    quarter of one KITTI 16-bit step (1/256 px)."""
    for (h, w), (fh, fw) in (((321, 1025), (375, 1242)), ((369, 1257), (375, 1242)), ((257, 513), (376, 672))):
        yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        px = (190.0 * xx / (w - 1) + 3.0 * np.sin(xx / 40.0) * np.cos(yy / 25.0) + 3.0).astype(f32)[None, None]
        got = to_frame(px, None, fh, fw, PIXELS)["out"]
        ref = torch.nn.functional.interpolate(torch.from_numpy(px) * (fw / w), size=(fh, fw), mode="bilinear", align_corners=False).numpy()
        err = np.abs(got.astype(np.float64) - ref).max()
        print("to_frame vs torch bilinear %dx%d -> %dx%d: max |diff| = %.3g px" % (w, h, fw, fh, err))
        assert err <= 1e-3, err


def test_back_end_matches_torch_bilinear_on_the_device(backend):
    d = Bufs(backend.name == "gpu")
    h, w, fh, fw = 161, 513, 375, 1242
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    px = (190.0 * xx / (w - 1) + 3.0 * np.sin(xx / 40.0) * np.cos(yy / 25.0) + 3.0).astype(f32)[None, None]
    got = run_to_frame(backend, d, px, None, fh, fw, PIXELS)["out"]
    ref = torch.nn.functional.interpolate(torch.from_numpy(px) * (fw / w), size=(fh, fw), mode="bilinear", align_corners=False).numpy()
    err = np.abs(got.astype(np.float64) - ref).max()
    assert err <= 1e-3, err


# ---- 4. refusals of both ops ------------------------------------------------------------------------------------------------------------
def test_front_end_refusals(backend):
    """factor 7 either way, a short step, an unknown encoding, null pointers, batch 0: RtError and nothing written"""
    d = Bufs(backend.name == "gpu")
    k = backend.klib
    src = d.put(pack(images(1, 70, 70, 5), capi.RT_ENC_BGRA8))
    E = capi.RT_ENC_BGRA8
    for twin in (0, 1):
        ol, orr = d.nan(2, 3, 490, 80), d.nan(2, 3, 490, 80)
        cases = [
            (src, src, 70, 70, 280, E, ol, orr, 80, 10, 1),            # x shrinks by 7 while y grows
            (src, src, 70, 70, 280, E, ol, orr, 10, 80, 1),            # y shrinks by 7 while x grows
            (src, src, 70, 70, 280, E, ol, orr, 10, 10, 1),            # both shrink by 7 (the box filter's limit)
            (src, src, 10, 10, 280, E, ol, orr, 80, 70, 1),            # y grows by 8, x by 7
            (src, src, 70, 10, 280, E, ol, orr, 70, 71, 1),            # x grows by 7.1
            (src, src, 70, 70, 279, E, ol, orr, 80, 80, 1),            # step shorter than 70 pixels of 4 bytes
            (src, src, 70, 70, 209, capi.RT_ENC_BGR8, ol, orr, 80, 80, 1),
            (src, src, 70, 70, 280, 4, ol, orr, 80, 80, 1),            # unknown encodings
            (src, src, 70, 70, 280, -1, ol, orr, 80, 80, 1),
            (None, src, 70, 70, 280, E, ol, orr, 80, 80, 1),           # null pointers
            (src, None, 70, 70, 280, E, ol, orr, 80, 80, 1),
            (src, src, 70, 70, 280, E, None, orr, 80, 80, 1),
            (src, src, 70, 70, 280, E, ol, None, 80, 80, 1),
            (src, src, 70, 70, 280, E, ol, orr, 80, 80, 0),            # batch < 1
            (src, src, 70, 70, 280, E, ol, orr, 0, 80, 1),             # sizes < 1
        ]
        for i, args in enumerate(cases):
            with pytest.raises(capi.RtError):
                k.preprocess_frames_u8_cv(*args, mirror_twin=twin)
            assert np.isnan(d.get(ol)).all() and np.isnan(d.get(orr)).all(), (twin, i)
        k.preprocess_frames_u8_cv(src, src, 70, 70, 280, E, ol, orr, 420, 80, 1, mirror_twin=twin)       # factor 6 next to them works
        got = d.get(ol).reshape(-1)
        assert not np.isnan(got[:(2 if twin else 1) * 3 * 420 * 80]).any()


def test_back_end_refusals(backend):
    d = Bufs(backend.name == "gpu")
    k = backend.klib
    px, mask = disparity_field(1, 10, 12, seed=13, with_mask=True)
    dpx, dm = d.put(px), d.put(mask)
    out, om, cnt = d.nan(1, 1, 70, 84), d.full((1, 1, 70, 84), np.uint8, 7), d.full((1,), np.uint64, 12345)
    cases = [
        ((dpx, 1, 10, 12, out, 71, 84), dict(mask=dm, out_mask=om, valid_count=cnt)),              # y grows by 7.1
        ((dpx, 1, 10, 12, out, 60, 85), dict(mask=dm, out_mask=om, valid_count=cnt)),              # x grows by more than 7
        ((dpx, 1, 70, 12, out, 10, 12), dict()),                                                   # y shrinks by 7
        ((dpx, 1, 10, 84, out, 10, 12), dict()),                                                   # x shrinks by 7
        ((dpx, 1, 10, 12, out, 20, 24), dict(kind=NET)),                                           # unknown kinds
        ((dpx, 1, 10, 12, out, 20, 24), dict(kind=3)),
        ((None, 1, 10, 12, out, 20, 24), dict()),                                                  # null pointers
        ((dpx, 1, 10, 12, None, 20, 24), dict()),
        ((dpx, 1, 10, 12, out, 20, 24), dict(out_mask=om)),                                        # mask outputs without a mask
        ((dpx, 1, 10, 12, out, 20, 24), dict(valid_count=cnt)),
        ((dpx, 0, 10, 12, out, 20, 24), dict()),                                                   # sizes < 1
        ((dpx, 1, 10, 12, out, 0, 24), dict()),
        ((dpx, 1, 10, 0, out, 20, 24), dict()),
    ]
    for i, (args, kw) in enumerate(cases):
        with pytest.raises(capi.RtError):
            k.disparity_to_frame(*args, **kw)
        assert np.isnan(d.get(out)).all() and (d.get(om, np.uint8) == 7).all() and (d.get(cnt, np.uint64) == 12345).all(), i
    k.disparity_to_frame(dpx, 1, 10, 12, out, 60, 72, mask=dm, out_mask=om, valid_count=cnt)         # factor 6 next to them works
    ref = to_frame(px, mask, 60, 72, PIXELS)
    assert np.array_equal(d.get(out).reshape(-1)[:60 * 72], ref["out"].reshape(-1))
    assert np.array_equal(d.get(cnt, np.uint64), ref["valid_count"])


# ---- 5. / 6. rt_net_execute_frames_ex on synthetic weights ---------------------------------------------------------------------------------
def outputs(d, n, h, w, kind):
    return dict(out=d.full((n, 1, h, w), np.uint16, 0xFFFF) if kind == U16 else d.nan(n, 1, h, w), mask=d.full((n, 1, h, w), np.uint8, 7),
                valid_count=d.full((n,), np.uint64, 12345))


def read(d, bufs, kind):
    types = dict(out=np.uint16 if kind == U16 else f32, mask=np.uint8, valid_count=np.uint64)
    return {key: d.get(v, types[key]) for key, v in bufs.items() if v is not None}


def untouched(d, bufs, kind):
    got = read(d, bufs, kind)
    return ((got["out"] == 0xFFFF).all() if kind == U16 else np.isnan(got["out"]).all()) and (got["mask"] == 7).all() and \
        (got["valid_count"] == 12345).all()


def engine_by_hand(lib, d, net, fl, fr, sh, sw, step, enc, h, w, n, check):
    """front end and engine of the pipeline by hand: the engine's raw (n or 2n, 1, h, w) output (the same for every kind and geometry)"""
    m = 2 * n if check else n
    il, ir, raw = d.nan(m, 3, h, w), d.nan(m, 3, h, w), d.nan(m, 1, h, w)
    lib.kernels.preprocess_frames_u8_cv(fl, fr, sh, sw, step, enc, il, ir, h, w, n, mirror_twin=check)
    net.execute(il, ir, raw, m)
    return raw


def by_hand(lib, d, net, fl, fr, sh, sw, step, enc, h, w, scale, n, kind, geometry, max_diff, raw=None):
    """the op-level calls a caller would write around rt_net_execute: the definition of rt_net_execute_frames_ex"""
    k = lib.kernels
    check = max_diff >= 0
    if raw is None:
        raw = engine_by_hand(lib, d, net, fl, fr, sh, sw, step, enc, h, w, n, check)
    oh, ow = (sh, sw) if geometry == G_FRAME else (h, w)
    bufs = outputs(d, n, oh, ow, kind)
    if not check:
        bufs["mask"] = bufs["valid_count"] = None
    if geometry == G_NET:
        if check:
            k.lr_consistency(raw, n, h, w, float(scale), max_diff, bufs["out"], kind, bufs["mask"], None, bufs["valid_count"])
        elif kind == NET:
            bufs["out"] = raw
        elif kind == PIXELS:
            k.disparity_scale(raw, bufs["out"], n * h * w, float(scale))
        else:
            k.disparity_to_u16(raw, bufs["out"], n * h * w, 256.0 * scale)
    elif check:
        px, m8 = d.nan(n, 1, h, w), d.full((n, 1, h, w), np.uint8, 7)
        k.lr_consistency(raw, n, h, w, float(scale), max_diff, px, PIXELS, m8, None, None)
        k.disparity_to_frame(px, n, h, w, bufs["out"], oh, ow, kind=kind, mask=m8, out_mask=bufs["mask"], valid_count=bufs["valid_count"])
    else:
        px = raw
        if scale != 1:
            px = d.nan(n, 1, h, w)
            k.disparity_scale(raw, px, n * h * w, float(scale))
        k.disparity_to_frame(px, n, h, w, bufs["out"], oh, ow, kind=kind)
    return read(d, bufs, kind)


def call_ex(d, net, fl, fr, enc, n, oh, ow, kind, geometry, resize, max_diff, bufs=None, **kw):
    bufs = bufs or outputs(d, n, oh, ow, kind)
    check = max_diff >= 0
    net.execute_frames_ex(fl, fr, enc, bufs["out"], kind=kind, geometry=geometry, resize=resize, max_diff_px=max_diff,
                          mask=bufs["mask"] if check else None, valid_count=bufs["valid_count"] if check else None, batch=n, **kw)
    return bufs


NETS = [("resnet18_2D", 0), ("resnet18_2D", capi.RT_CONV_EXACT_FP32), ("nvtiny", 0)]
NET_IDS = ["resnet18_2D", "resnet18_2D-exact", "nvtiny"]


@pytest.mark.parametrize("sh,sw", [(30, 36), (20, 83)], ids=["36x30", "83x20"])
@pytest.mark.parametrize("model,flags", NETS, ids=NET_IDS)
def test_execute_frames_ex_equals_the_pipeline_by_hand(rt, model, flags, sh, sw):
    """frames 36 x 30 (x grows, y shrinks) and 83 x 20 (the other way) into 41 x 25 / 33 x 25 nets: every (kind, geometry, check)
    combination bit-equal to the op-level calls; RT_GEOM_FRAME + RT_DISP_NET refused"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    net, h, w, scale = make_net(lib, model, flags)
    n, enc = (2 if flags else 1), capi.RT_ENC_BGRA8        # (two pairs on the exact-fp32 engine only: the others are slow on the emulator)
    fl, fr = d.put(pack(images(n, sh, sw, 21), enc, PAD, 11)), d.put(pack(images(n, sh, sw, 22), enc, PAD, 12))
    step = fl.shape[2]
    raws = {check: engine_by_hand(lib, d, net, fl, fr, sh, sw, step, enc, h, w, n, check) for check in (False, True)}
    for geometry in (G_NET, G_FRAME):
        oh, ow = (sh, sw) if geometry == G_FRAME else (h, w)
        for max_diff in (-1.0, 1.5):
            for kind in (NET, PIXELS, U16):
                what = (geometry, max_diff, kind)
                if geometry == G_FRAME and kind == NET:
                    bufs = outputs(d, n, oh, ow, kind)
                    with pytest.raises(capi.RtError) as e:
                        call_ex(d, net, fl, fr, enc, n, oh, ow, kind, geometry, CV, max_diff, bufs=bufs, src_w=sw)
                    assert "(%d)" % -2 in str(e.value) and untouched(d, bufs, kind), str(e.value)        # RT_E_UNSUPPORTED
                    continue
                ref = by_hand(lib, d, net, fl, fr, sh, sw, step, enc, h, w, scale, n, kind, geometry, max_diff, raw=raws[max_diff >= 0])
                got = read(d, call_ex(d, net, fl, fr, enc, n, oh, ow, kind, geometry, CV, max_diff, src_w=sw), kind)
                if max_diff < 0:
                    got = dict(out=got["out"])                 # mask and count were not passed: still at their sentinels, checked below
                assert not np.isnan(ref["out"].astype(np.float64)).any(), what
                assert_same(got, ref, what)
                if max_diff >= 0:
                    assert 0 < ref["valid_count"].sum() < n * oh * ow, what
    # a wrong struct size, bad enum values, a NaN tolerance, mask outputs without a check, too large a batch: error, nothing written
    bufs = outputs(d, n, sh, sw, PIXELS)
    big_l, big_r = d.put(pack(images(5, sh, sw, 1), enc)), d.put(pack(images(5, sh, sw, 2), enc))
    bad = [dict(struct_bytes=ctypes.sizeof(capi.FrameCall) - 8), dict(struct_bytes=0), dict(resize=2), dict(resize=-1), dict(geometry=2),
           dict(geometry=-1), dict(kind=3), dict(kind=-1), dict(max_diff_px=float("nan")), dict(max_diff_px=-1.0, mask=bufs["mask"]),
           dict(max_diff_px=-1.0, valid_count=bufs["valid_count"]), dict(batch=3, max_diff_px=1.0, fl=big_l, fr=big_r), dict(batch=5, fl=big_l, fr=big_r),
           dict(batch=0), dict(encoding=9)]
    for kw in bad:
        args = dict(kind=PIXELS, geometry=G_FRAME, resize=CV, max_diff_px=-1.0, batch=n, src_w=sw)
        args.update(kw)
        a, b, e = args.pop("fl", fl), args.pop("fr", fr), args.pop("encoding", enc)
        with pytest.raises(capi.RtError):
            net.execute_frames_ex(a, b, e, bufs["out"], **args)
        assert untouched(d, bufs, PIXELS), kw
    with pytest.raises(capi.RtError):
        net.execute_frames_ex(fl, fr, enc, None, src_w=sw, batch=n)
    net.destroy()


@pytest.mark.parametrize("model,flags", NETS, ids=NET_IDS)
def test_execute_frames_ex_area_down_net_geometry_is_the_existing_call(rt, model, flags):
    """on an 83 x 51 frame bit-equal to execute_frames and execute_frames_lr for all three kinds; a 30 x 20 frame is refused as they
    refuse it, nothing written; the net alternates between old and new calls"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    net, h, w, scale = make_net(lib, model, flags)
    n, enc = (2 if flags else 1), capi.RT_ENC_BGRA8        # (two pairs on the exact-fp32 engine only: the others are slow on the emulator)
    fl, fr = d.put(pack(images(n, 51, 83, 21), enc, PAD, 11)), d.put(pack(images(n, 51, 83, 22), enc, PAD, 12))
    small = d.put(pack(images(n, 20, 30, 1), capi.RT_ENC_BGR8))
    for kind in (NET, PIXELS, U16):
        old = outputs(d, n, h, w, kind)
        net.execute_frames(fl, fr, enc, old["out"], kind=kind, batch=n, src_w=83)
        new = read(d, call_ex(d, net, fl, fr, enc, n, h, w, kind, G_NET, DOWN, -1.0, src_w=83), kind)
        assert np.array_equal(new["out"], read(d, old, kind)["out"]) and not np.isnan(new["out"].astype(np.float64)).any(), kind
        # the same frames through the full filter: neither axis grows, so it is the same front end
        if kind == PIXELS:
            cv = read(d, call_ex(d, net, fl, fr, enc, n, h, w, kind, G_NET, CV, -1.0, src_w=83), kind)
            assert np.array_equal(cv["out"], new["out"]), kind
        old = outputs(d, n, h, w, kind)
        net.execute_frames_lr(fl, fr, enc, old["out"], kind=kind, mask=old["mask"], valid_count=old["valid_count"], max_diff_px=1.0, batch=n,
                              src_w=83)
        new = read(d, call_ex(d, net, fl, fr, enc, n, h, w, kind, G_NET, DOWN, 1.0, src_w=83), kind)
        assert_same(new, read(d, old, kind), kind)
        for max_diff in (-1.0, 1.0):
            bufs = outputs(d, n, h, w, kind)
            with pytest.raises(capi.RtError) as e_new:
                call_ex(d, net, small, small, capi.RT_ENC_BGR8, n, h, w, kind, G_NET, DOWN, max_diff, bufs=bufs, src_w=30)
            assert untouched(d, bufs, kind)
            with pytest.raises(capi.RtError) as e_old:
                if max_diff < 0:
                    net.execute_frames(small, small, capi.RT_ENC_BGR8, bufs["out"], kind=kind, batch=n, src_w=30)
                else:
                    net.execute_frames_lr(small, small, capi.RT_ENC_BGR8, bufs["out"], kind=kind, mask=bufs["mask"],
                                          valid_count=bufs["valid_count"], max_diff_px=max_diff, batch=n, src_w=30)
            assert str(e_new.value).split("failed", 1)[1] == str(e_old.value).split("failed", 1)[1]        # same code, same message
            # ... and RT_GEOM_FRAME does not lift the refusal of the down-only filter
            with pytest.raises(capi.RtError):
                call_ex(d, net, small, small, capi.RT_ENC_BGR8, n, h, w, kind if kind != NET else PIXELS, G_FRAME, DOWN, max_diff, bufs=bufs,
                        src_w=30)
            assert untouched(d, bufs, kind)
    net.destroy()


# ---- 7. GPU only: the reference's sample pair and trained weights ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_sample_pair_into_the_headline_network():
    """the reference's own 1242 x 375 bgr8 pair into ResNet-18 2D 1257 x 369 fp32 (the timed configuration): network-geometry pixels
    within 1e-3 * w of the oracle network run on the numpy-restated pre-processing; frame-geometry output bit-equal to
    rt_disparity_to_frame of them"""
    lib, d = netlib("gpu"), Bufs(True)
    w, h = 1257, 369
    net = lib.create("resnet18_2D", w, h, max_batch=2, weights_path=model_files.weight_file("resnet18_2D"))
    left, right = sample_bgr()
    sh, sw = left.shape[1:3]
    assert (sh, sw) == (375, 1242)
    fl, fr = d.put(pack(left, capi.RT_ENC_BGR8)), d.put(pack(right, capi.RT_ENC_BGR8))
    px = read(d, call_ex(d, net, fl, fr, capi.RT_ENC_BGR8, 1, h, w, PIXELS, G_NET, CV, -1.0, src_w=sw), PIXELS)["out"]
    l, r = cv_planes(left, h, w), cv_planes(right, h, w)
    with torch.no_grad():
        ref = O.resnet18_2d(torch.from_numpy(l), torch.from_numpy(r), O.read_weights(model_files.weight_file("resnet18_2D"))).numpy()
    err = np.abs(px - ref * w).max()
    print("execute_frames_ex resnet18_2D 1257x369 fp32 on the 1242x375 sample pair: max |px - oracle px| = %.3g (bound %.3g), max disparity %.1f px"
          % (err, 1e-3 * w, px.max()))
    assert err <= 1e-3 * w, err
    for kind in (PIXELS, U16):
        got = read(d, call_ex(d, net, fl, fr, capi.RT_ENC_BGR8, 1, sh, sw, kind, G_FRAME, CV, -1.0, src_w=sw), kind)["out"]
        want = run_to_frame(_Klib(lib), d, px, None, sh, sw, kind)["out"]
        assert got.shape == (1, 1, sh, sw) and np.array_equal(got, want), kind
        assert np.array_equal(want, to_frame(px, None, sh, sw, kind)["out"]), kind
    # with a check: bit-equal to the pipeline by hand
    ref = by_hand(lib, d, net, fl, fr, sh, sw, 3 * sw, capi.RT_ENC_BGR8, h, w, w, 1, PIXELS, G_FRAME, 1.0)
    got = read(d, call_ex(d, net, fl, fr, capi.RT_ENC_BGR8, 1, sh, sw, PIXELS, G_FRAME, CV, 1.0, src_w=sw), PIXELS)
    assert_same(got, ref)
    print("left-right check at 1 px in frame geometry keeps %.1f %% of the sample frame" % (100.0 * got["valid_count"][0] / (sh * sw)))
    assert 0 < got["valid_count"][0] < sh * sw                   # neither everything nor nothing
    net.destroy()


class _Klib:
    """run_to_frame takes a backend: the kernel library of a NetLib in that role"""

    def __init__(self, lib):
        self.klib = lib.kernels


@pytest.mark.gpu
def test_reference_sample_pair_nvtiny_shrinks_both_ways():
    """1242 x 375 into nvtiny 513 x 161: neither axis grows, so RT_RESIZE_CV_AREA is bit-equal to execute_frames"""
    lib, d = netlib("gpu"), Bufs(True)
    net = lib.create("nvtiny", 513, 161, weights_path=model_files.weight_file("nvtiny"))
    left, right = sample_bgr()
    fl, fr = d.put(pack(left, capi.RT_ENC_BGR8)), d.put(pack(right, capi.RT_ENC_BGR8))
    for kind in (NET, PIXELS, U16):
        old = outputs(d, 1, 161, 513, kind)
        net.execute_frames(fl, fr, capi.RT_ENC_BGR8, old["out"], kind=kind, batch=1, src_w=1242)
        new = read(d, call_ex(d, net, fl, fr, capi.RT_ENC_BGR8, 1, 161, 513, kind, G_NET, CV, -1.0, src_w=1242), kind)
        assert np.array_equal(new["out"], read(d, old, kind)["out"]), kind
    net.destroy()


# ---- 8. GPU only: graph mode with rotating buffers -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("streams", [2, 1])
def test_graph_mode_with_rotating_buffers_frame_geometry_and_check(streams):
    """a camera ring: three sets of frame, disparity, mask and count buffers in rotation, on a torch stream and on the NULL stream, graph
    mode on, RT_GEOM_FRAME with a check -- every rotation bit-equal to the non-graph result"""
    lib, d = netlib("gpu"), Bufs(True)
    h, w, n, sh, sw = 129, 257, 2, 120, 300                  # x shrinks, y grows
    net = lib.create("resnet18_2D", w, h, max_batch=2 * n, weights=O.synth_weights_resnet18_2d(), max_disp=16)
    net.set_streams(streams)
    enc, kind = capi.RT_ENC_BGRA8, PIXELS
    sets = [(d.put(pack(images(n, sh, sw, 40 + 2 * i), enc, PAD, i)), d.put(pack(images(n, sh, sw, 41 + 2 * i), enc, PAD, i + 7))) for i in range(3)]

    def run(i, bufs, stream=None):
        call_ex(d, net, sets[i][0], sets[i][1], enc, n, sh, sw, kind, G_FRAME, CV, 1.0, bufs=bufs, src_w=sw, stream=stream)

    direct = []
    for i in range(3):
        bufs = outputs(d, n, sh, sw, kind)
        run(i, bufs)
        direct.append(read(d, bufs, kind))
    assert not np.isnan(direct[0]["out"]).any() and not np.array_equal(direct[0]["out"], direct[1]["out"])
    assert_same(direct[0], by_hand(lib, d, net, sets[0][0], sets[0][1], sh, sw, sets[0][0].shape[2], enc, h, w, w, n, kind, G_FRAME, 1.0))
    net.set_graph(True)
    ring = [outputs(d, n, sh, sw, kind) for _ in range(3)]
    s = torch.cuda.Stream()
    for call in range(9):                                 # 1: direct, 2: capture + launch, then replays, whatever pointers rotate in
        i = call % 3
        ring[i]["out"].fill_(float("nan"))
        ring[i]["mask"].fill_(7)
        ring[i]["valid_count"].fill_(12345)
        torch.cuda.synchronize()
        run(i, ring[i], stream=s.cuda_stream)
        s.synchronize()
        assert_same(read(d, ring[i], kind), direct[i], call)
    for call in range(6):
        i = (call + 1) % 3
        ring[i]["out"].fill_(float("nan"))
        torch.cuda.synchronize()
        run(i, ring[i])
        assert_same(read(d, ring[i], kind), direct[i], call)
    net.destroy()
