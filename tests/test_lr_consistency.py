"""Left-right consistency check on the camera-frame path.

A left-referenced network gives the right view's disparity when it is fed the mirrored right image as "left" and the mirrored left image
as "right".  Three entries do that inside one engine batch:

- rt_preprocess_frames_u8_lr: rt_preprocess_frames_u8 into images [0, N) of two batches of 2N images, plus the mirrored, swapped pair as
  images [N, 2N).  Bit-identical to rt_preprocess_frames_u8 and to the numpy flip-and-swap of its output.
- rt_lr_consistency: the check, the mask and the output encoding of the engine's (2N,1,H,W) output.  All fp32, each operation rounded on
  its own, so `restate` below (numpy float32) is bit-exact: no tolerance anywhere in the kernel-level cases.
- rt_net_execute_frames_lr: the two around one engine pass at batch 2N, bit-equal to the manual pipeline on the same engine.
CPU tier: the same sources on the SIMT emulator; GPU tier (-m gpu): the MI355X, plus the reference's sample pair with trained weights."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import stereo_oracle as O
from redtail_amd import capi, model_files
from test_camera_frames import ENCODINGS, PAD, Dev, images, netlib, pack, rt, sample_bgr  # noqa: F401  (rt: the emu / gpu fixture)

KINDS = [capi.RT_DISP_NET, capi.RT_DISP_PIXELS_F32, capi.RT_DISP_KITTI_U16]
KIND_IDS = ["net", "pixels", "kitti-u16"]


# ---- the check restated in numpy float32 ------------------------------------------------------------------------------------------------
def views(net, batch, scale):
    """(dL, dR, raw L, raw un-mirrored R) of a (2N,1,H,W) engine output: pixels = raw * scale, one float32 multiply"""
    net = np.asarray(net, np.float32)
    s = np.float32(scale)
    raw_l, raw_r = net[:batch, 0], net[batch:, 0, :, ::-1]
    return raw_l * s, raw_r * s, raw_l, raw_r


def match(d_l, d_r):
    """xr = rint(x - dL) (float32, ties to even), whether it lies in the right view, and dR(xr) there"""
    w = d_l.shape[-1]
    x = np.arange(w, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        xr = np.rint(x - d_l)
        inview = (xr >= 0) & (xr <= np.float32(w - 1))           # False for NaN
    gathered = np.take_along_axis(d_r, np.where(inview, xr, 0).astype(np.int64), axis=-1)
    return xr, inview, gathered


def to_u16(raw, scale):
    with np.errstate(invalid="ignore"):
        return np.clip(np.rint(raw * (np.float32(256) * np.float32(scale))), 0, 65535).astype(np.uint16)


def restate(net, batch, scale, max_diff, kind):
    """what rt_lr_consistency must write, bit for bit: out, mask, right_out, valid_count"""
    d_l, d_r, raw_l, raw_r = views(net, batch, scale)
    _, inview, g = match(d_l, d_r)
    with np.errstate(invalid="ignore"):
        valid = inview & (np.abs(d_l - g) <= np.float32(max_diff))
    if kind == capi.RT_DISP_NET:
        enc_l, enc_r = raw_l, raw_r
    elif kind == capi.RT_DISP_PIXELS_F32:
        enc_l, enc_r = d_l, d_r
    else:
        enc_l, enc_r = np.maximum(to_u16(raw_l, scale), 1), to_u16(raw_r, scale)      # a valid 0 is raised to 1; the right view is not masked
    out = np.where(valid, enc_l, enc_l.dtype.type(0))
    return dict(out=out[:, None], mask=(valid * np.uint8(255))[:, None], right_out=np.ascontiguousarray(enc_r)[:, None],
                valid_count=valid.sum(axis=(1, 2)).astype(np.uint64))


def undecidable(net, batch, scale, max_diff, margin):
    """pixels whose verdict a perturbation of `margin` px of the disparities can flip: x - dL within `margin` of a rounding tie, or
    |dL - dR(xr)| within `margin` of the threshold"""
    d_l, d_r, _, _ = views(net, batch, scale)
    _, inview, g = match(d_l, d_r)
    t = np.arange(d_l.shape[-1], dtype=np.float64) - d_l.astype(np.float64)
    near_tie = np.abs((t - np.floor(t)) - 0.5) < margin
    near_thr = inview & (np.abs(np.abs(d_l.astype(np.float64) - g) - max_diff) < margin)
    return (near_tie | near_thr)[:, None]


# ---- buffers -------------------------------------------------------------------------------------------------------------------------------
class Bufs(Dev):
    """Dev plus the integer buffers of the check, pre-filled so that an element left unwritten shows"""

    def full(self, shape, dtype, value):
        a = np.full(shape, value, dtype)
        if not self.gpu:
            return a
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint64): np.int64}.get(a.dtype)
        return torch.from_numpy(a.view(signed) if signed else a).cuda()

    def get(self, t, dtype=None):
        a = super().get(t)
        return a.view(dtype) if dtype is not None and a.dtype != np.dtype(dtype) else a

    def outputs(self, n, h, w, kind):
        out = self.full((n, 1, h, w), np.uint16, 0xFFFF) if kind == capi.RT_DISP_KITTI_U16 else self.nan(n, 1, h, w)
        rout = self.full((n, 1, h, w), np.uint16, 0xFFFF) if kind == capi.RT_DISP_KITTI_U16 else self.nan(n, 1, h, w)
        return dict(out=out, mask=self.full((n, 1, h, w), np.uint8, 7), right_out=rout, valid_count=self.full((n,), np.uint64, 12345))

    def read(self, bufs, kind):
        dt = np.uint16 if kind == capi.RT_DISP_KITTI_U16 else np.float32
        types = dict(out=dt, mask=np.uint8, right_out=dt, valid_count=np.uint64)
        return {k: self.get(v, types[k]) for k, v in bufs.items() if v is not None}


def run_check(backend, d, net, batch, scale, max_diff, kind, want=("mask", "right_out", "valid_count"), stream=None):
    n2, _, h, w = net.shape
    bufs = d.outputs(batch, h, w, kind)
    for k in ("mask", "right_out", "valid_count"):
        if k not in want:
            bufs[k] = None
    backend.klib.lr_consistency(d.put(net), batch, h, w, float(scale), float(max_diff), bufs["out"], kind, bufs["mask"], bufs["right_out"],
                                bufs["valid_count"], stream=stream)
    return d.read(bufs, kind)


def assert_equal(got, ref, what=""):
    for k, v in got.items():
        assert v.dtype == ref[k].dtype and v.shape == ref[k].shape, (what, k, v.dtype, v.shape)
        assert np.array_equal(v, ref[k]), (what, k, int((v != ref[k]).sum()))        # NaN-free where it matters: array_equal fails on NaN


# ---- 1. front end: rt_preprocess_frames_u8_lr -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3], ids=["b1", "b3"])
@pytest.mark.parametrize("pad", [0, PAD], ids=["dense", "pitched"])
@pytest.mark.parametrize("encoding", ENCODINGS, ids=["bgr8", "rgb8", "bgra8", "rgba8"])
@pytest.mark.parametrize("src,dst", [((37, 59), (37, 59)), ((60, 300), (31, 161)), ((50, 200), (23, 130))],
                         ids=["same-59", "odd-161", "even-130"])
def test_front_end_equals_preprocess_frames_and_its_flip(backend, src, dst, encoding, pad, n):
    d = Dev(backend.name == "gpu")
    left, right = images(n, *src, seed=3), images(n, *src, seed=4)
    fl, fr = d.put(pack(left, encoding, pad, 1)), d.put(pack(right, encoding, pad, 2))
    step = fl.shape[2]
    ol, orr = d.nan(2 * n, 3, *dst), d.nan(2 * n, 3, *dst)
    backend.klib.preprocess_frames_u8_lr(fl, fr, src[0], src[1], step, encoding, ol, orr, dst[0], dst[1], n)
    rl, rr = d.nan(n, 3, *dst), d.nan(n, 3, *dst)
    backend.klib.preprocess_frames_u8(fl, fr, src[0], src[1], step, encoding, rl, rr, dst[0], dst[1], n)
    got_l, got_r, ref_l, ref_r = d.get(ol), d.get(orr), d.get(rl), d.get(rr)
    assert not np.isnan(ref_l).any() and not np.isnan(ref_r).any()
    assert np.array_equal(got_l[:n], ref_l) and np.array_equal(got_r[:n], ref_r)
    assert np.array_equal(got_l[n:], ref_r[..., ::-1])           # mirrored and swapped
    assert np.array_equal(got_r[n:], ref_l[..., ::-1])


def test_front_end_refusals(backend):
    """the refusals of rt_preprocess_frames_u8: RtError, and nothing is written"""
    d = Dev(backend.name == "gpu")
    k = backend.klib
    src = d.put(pack(images(1, 70, 70, 5), capi.RT_ENC_BGRA8))
    ol, orr = d.nan(2, 3, 80, 80), d.nan(2, 3, 80, 80)
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
            k.preprocess_frames_u8_lr(*args, 1)
        assert np.isnan(d.get(ol)).all() and np.isnan(d.get(orr)).all(), i
    k.preprocess_frames_u8_lr(src, src, 70, 70, 280, capi.RT_ENC_BGRA8, ol, orr, 35, 35, 1)   # and the valid call next to them works
    assert not np.isnan(d.get(ol).reshape(-1)[:2 * 3 * 35 * 35]).any()


# ---- 2. the check on fields whose answer is known -----------------------------------------------------------------------------------------
def two_views(d_l, d_r):
    """(2N,1,H,W) engine output (scale 1) from left-view and right-view disparities in pixels: the second half is stored mirrored"""
    return np.concatenate([d_l, d_r[..., ::-1]]).astype(np.float32)[:, None]


def bar_scene(h=6, w=97):
    """background 3 px, a foreground bar of 12 px over left columns 40..60 = right-view columns 28..48"""
    d_l, d_r = np.full((1, h, w), 3, np.float32), np.full((1, h, w), 3, np.float32)
    d_l[..., 40:61] = 12
    d_r[..., 28:49] = 12
    return d_l, d_r


def test_check_bar_scene(backend):
    """invalid are exactly columns 0..2 (outside the right view) and 31..39 (the strip the bar occludes, 12 - 3 = 9 wide)"""
    d = Bufs(backend.name == "gpu")
    h, w = 6, 97
    net = two_views(*bar_scene(h, w))
    invalid = np.zeros(w, bool)
    invalid[0:3] = invalid[31:40] = True
    for kind in KINDS:
        got = run_check(backend, d, net, 1, 1.0, 1.0, kind)
        assert np.array_equal(got["mask"][0, 0], np.broadcast_to(np.where(invalid, 0, 255).astype(np.uint8), (h, w))), kind
        assert got["valid_count"].tolist() == [h * 85]
        assert_equal(got, restate(net, 1, 1.0, 1.0, kind), kind)
        assert (got["out"][0, 0][:, invalid] == 0).all() and (got["out"][0, 0][:, ~invalid] != 0).all()


def test_check_nan_invalidates_the_pixels_that_read_it(backend):
    d = Bufs(backend.name == "gpu")
    h, w = 6, 97
    d_l, d_r = bar_scene(h, w)
    base = restate(two_views(d_l, d_r), 1, 1.0, 1.0, capi.RT_DISP_PIXELS_F32)["mask"][0, 0] == 255
    d_l[0, 2, 70] = np.nan            # left view: pixel (2, 70) itself
    d_r[0, 4, 10] = np.nan            # right view, background: read by left pixel x = 10 + 3
    d_r[0, 1, 30] = np.nan            # right view, inside the bar: read by left pixel x = 30 + 12
    d_r[0, 5, 96] = np.nan            # right view's last column: no left pixel maps there (96 + 3 > 96)
    expect = base.copy()
    expect[2, 70] = expect[4, 13] = expect[1, 42] = False
    net = two_views(d_l, d_r)
    got = run_check(backend, d, net, 1, 1.0, 1.0, capi.RT_DISP_PIXELS_F32)
    assert np.array_equal(got["mask"][0, 0] == 255, expect)
    assert got["valid_count"].tolist() == [int(expect.sum())]
    assert np.array_equal(got["out"][0, 0], np.where(expect, np.nan_to_num(d_l[0]), 0))
    assert np.array_equal(got["right_out"][0, 0], d_r[0], equal_nan=True)              # unmasked: the NaNs pass through


def test_check_zero_tolerance_and_ties(backend):
    d = Bufs(backend.name == "gpu")
    h, w = 4, 97
    cols = np.arange(w)
    # equal views, max_diff 0: every pixel whose match lies in the right view stays.  2.25: x = 2 maps to rint(-0.25) = -0 = column 0
    for disp, first in ((4.0, 4), (2.25, 2), (0.0, 0)):
        net = two_views(np.full((1, h, w), disp, np.float32), np.full((1, h, w), disp, np.float32))
        got = run_check(backend, d, net, 1, 1.0, 0.0, capi.RT_DISP_PIXELS_F32)
        assert np.array_equal(got["mask"][0, 0] == 255, np.broadcast_to(cols >= first, (h, w))), disp
        assert_equal(got, restate(net, 1, 1.0, 0.0, capi.RT_DISP_PIXELS_F32), disp)
    # x - 2.5 is a tie for every x: ties to even reach the even right-view columns only (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0), which
    # alone hold a consistent value here; rounding half away from zero or half up would land on the odd ones
    d_r = np.where(cols % 2 == 0, np.float32(2.5), np.float32(100)) * np.ones((1, h, 1), np.float32)
    net = two_views(np.full((1, h, w), 2.5, np.float32), d_r)
    got = run_check(backend, d, net, 1, 1.0, 0.0, capi.RT_DISP_PIXELS_F32)
    assert np.array_equal(got["mask"][0, 0] == 255, np.broadcast_to(cols >= 2, (h, w)))
    assert got["valid_count"].tolist() == [h * (w - 2)]


def test_check_refusals(backend):
    """negative or NaN tolerance, unknown kind, empty dims, null net_disp / out: RtError and nothing written"""
    d = Bufs(backend.name == "gpu")
    k = backend.klib
    net = d.put(two_views(*bar_scene(6, 97)))
    bufs = d.outputs(1, 6, 97, capi.RT_DISP_PIXELS_F32)
    o, m, r, c = bufs["out"], bufs["mask"], bufs["right_out"], bufs["valid_count"]
    cases = [(net, 1, 6, 97, 1.0, -0.5, o, 1, m, r, c), (net, 1, 6, 97, 1.0, float("nan"), o, 1, m, r, c),
             (net, 1, 6, 97, 1.0, 1.0, o, 3, m, r, c), (net, 1, 6, 97, 1.0, 1.0, o, -1, m, r, c),
             (net, 0, 6, 97, 1.0, 1.0, o, 1, m, r, c), (net, 1, 0, 97, 1.0, 1.0, o, 1, m, r, c), (net, 1, 6, 0, 1.0, 1.0, o, 1, m, r, c),
             (None, 1, 6, 97, 1.0, 1.0, o, 1, m, r, c), (net, 1, 6, 97, 1.0, 1.0, None, 1, m, r, c)]
    for i, args in enumerate(cases):
        with pytest.raises(capi.RtError):
            k.lr_consistency(*args)
        got = d.read(bufs, capi.RT_DISP_PIXELS_F32)
        assert np.isnan(got["out"]).all() and np.isnan(got["right_out"]).all() and (got["mask"] == 7).all(), i
        assert got["valid_count"].tolist() == [12345], i


# ---- 3. random fields, bit-exact --------------------------------------------------------------------------------------------------------
def random_views(batch, h, w, scale, max_diff, seed):
    """(2N,1,H,W) engine output: a piecewise-smooth left disparity (pixels, up to W/8), the right view = the left one warped forward
    (nearest column, the nearer surface wins, holes filled at random) plus noise of the size of the tolerance; row 0: disparity 0 in both
    views, no noise (valid pixels whose 16-bit value is 0)"""
    rng = np.random.default_rng(seed)
    top = w / 8.0
    d_l = np.empty((batch, h, w), np.float32)
    for n in range(batch):
        for y in range(h):
            knots = np.sort(rng.integers(0, w, 4))
            level = rng.uniform(0, top, 5)
            d_l[n, y] = level[np.searchsorted(knots, np.arange(w), side="right")] + 0.02 * np.arange(w) / w
    d_l[:, 0] = 0
    d_r = np.full((batch, h, w), -1, np.float32)
    xr = np.rint(np.arange(w, dtype=np.float32) - d_l)
    ok = (xr >= 0) & (xr <= w - 1)
    nn, yy, _ = np.nonzero(ok)
    np.maximum.at(d_r, (nn, yy, xr[ok].astype(np.int64)), d_l[ok])
    holes = d_r < 0
    d_r[holes] = rng.uniform(0, top, int(holes.sum())).astype(np.float32)
    noise = rng.normal(0, 0.8 * max_diff, d_r.shape).astype(np.float32)
    noise[:, 0] = 0
    d_r = np.abs(d_r + noise)
    d_r[:, 0] = 0
    return (two_views(d_l, d_r) / np.float32(scale)).astype(np.float32)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("unit_scale", [True, False], ids=["scale-1", "scale-W"])
@pytest.mark.parametrize("batch", [1, 3], ids=["b1", "b3"])
@pytest.mark.parametrize("h,w", [(23, 97), (369, 1257), (161, 513)])
def test_check_random_fields_bit_exact(backend, h, w, batch, unit_scale, kind):
    d = Bufs(backend.name == "gpu")
    scale, max_diff = (1.0 if unit_scale else float(w)), 1.0
    net = random_views(batch, h, w, scale, max_diff, seed=h + batch)
    ref = restate(net, batch, scale, max_diff, kind)
    share = ref["valid_count"].sum() / float(batch * h * w)
    assert 0.2 <= share <= 0.8, share                            # a condition on the input, stated on the restatement alone
    if kind == capi.RT_DISP_KITTI_U16:
        valid = ref["mask"] == 255
        assert (to_u16(net[:batch], scale)[valid] == 0).any()    # the input holds valid pixels that encode to 0: they must come out as 1
    combos = [("mask", "right_out", "valid_count"), ()]
    if (h, w) == (23, 97):
        combos += [("right_out", "valid_count"), ("mask", "valid_count"), ("mask", "right_out"), ("mask",), ("right_out",), ("valid_count",)]
    for want in combos:
        got = run_check(backend, d, net, batch, scale, max_diff, kind, want)
        assert set(got) == {"out"} | set(want)
        assert_equal(got, ref, want)
        if kind == capi.RT_DISP_KITTI_U16 and "mask" in want:
            assert (got["out"][got["mask"] == 255] != 0).all() and (got["out"][got["mask"] == 0] == 0).all()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_check_on_views_off_a_16_byte_boundary(backend, kind):
    """every buffer 4 (the mask: 1, the 16-bit maps: 2) bytes past an aligned address: same result through the element-wise path"""
    d = Bufs(backend.name == "gpu")
    batch, h, w = 3, 23, 97
    net = random_views(batch, h, w, 1.0, 1.0, seed=5)
    ref = restate(net, batch, 1.0, 1.0, kind)
    src = d.put(np.concatenate([np.zeros(1, np.float32), net.reshape(-1)]))
    dt, fill = (np.uint16, 0xFFFF) if kind == capi.RT_DISP_KITTI_U16 else (np.float32, np.nan)
    n = batch * h * w
    out, rout, mask, cnt = d.full((n + 1,), dt, fill), d.full((n + 1,), dt, fill), d.full((n + 1,), np.uint8, 7), d.full((batch,), np.uint64, 9)
    backend.klib.lr_consistency(src[1:], batch, h, w, 1.0, 1.0, out[1:], kind, mask[1:], rout[1:], cnt)
    got = dict(out=d.get(out, dt), mask=d.get(mask, np.uint8), right_out=d.get(rout, dt), valid_count=d.get(cnt, np.uint64))
    for k in ("out", "mask", "right_out"):
        first = got[k][0]
        assert (np.isnan(first) if dt == np.float32 and k != "mask" else first == (7 if k == "mask" else fill)), k     # the element in front is untouched
        got[k] = got[k][1:].reshape(batch, 1, h, w)
    assert_equal(got, ref, kind)


# ---- 4. rt_net_execute_frames_lr on synthetic weights ---------------------------------------------------------------------------------------
def make_net(lib, model, flags=0, fp16=False, max_batch=4):
    if model == "resnet18_2D":
        h, w, weights, disp = 25, 41, O.synth_weights_resnet18_2d(), 8
    else:
        h, w, weights, disp = 25, 33, O.synth_weights_3d(O.NVTINY_3D), 4
    net = lib.create(model, w, h, max_batch=max_batch, weights=weights, max_disp=disp, flags=flags, fp16_weights=fp16)
    return net, h, w, (w if model == "resnet18_2D" else 1)


def manual_lr(lib, d, net, fl, fr, src_h, src_w, step, encoding, h, w, n):
    """rt_preprocess_frames_u8 -> flip and swap on the host -> rt_net_execute at batch 2N: the engine's raw (2N,1,h,w) output"""
    il, ir = d.nan(n, 3, h, w), d.nan(n, 3, h, w)
    lib.kernels.preprocess_frames_u8(fl, fr, src_h, src_w, step, encoding, il, ir, h, w, n)
    left, right = d.get(il), d.get(ir)
    out = d.nan(2 * n, 1, h, w)
    net.execute(d.put(np.concatenate([left, right[..., ::-1]])), d.put(np.concatenate([right, left[..., ::-1]])), out, 2 * n)
    raw = d.get(out)
    assert not np.isnan(raw).any()
    return raw


def call_lr(d, net, fl, fr, encoding, n, h, w, kind, max_diff, bufs=None, **kw):
    bufs = bufs or d.outputs(n, h, w, kind)
    net.execute_frames_lr(fl, fr, encoding, bufs["out"], kind=kind, mask=bufs["mask"], disp_right=bufs["right_out"],
                          valid_count=bufs["valid_count"], max_diff_px=max_diff, batch=n, **kw)
    return bufs


@pytest.mark.parametrize("model,flags,fp16", [("resnet18_2D", 0, False), ("resnet18_2D", capi.RT_CONV_EXACT_FP32, False),
                                              ("resnet18_2D", 0, True), ("nvtiny", 0, False)],
                         ids=["resnet18_2D", "resnet18_2D-exact", "resnet18_2D-half2", "nvtiny"])
def test_execute_frames_lr_equals_manual_pipeline(rt, model, flags, fp16):
    """bgra8 frames with a padded step from an 83x51 source, batch 2 of max_batch 4: every output of every kind bit-equal to the manual
    pipeline (which presumes that the engine's result for an image does not depend on its position in the batch)"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    net, h, w, scale = make_net(lib, model, flags, fp16)
    n, enc = 2, capi.RT_ENC_BGRA8
    left, right = images(n, 51, 83, 21), images(n, 51, 83, 22)
    fl, fr = d.put(pack(left, enc, PAD, 11)), d.put(pack(right, enc, PAD, 12))
    raw = manual_lr(lib, d, net, fl, fr, 51, 83, fl.shape[2], enc, h, w, n)
    for kind in KINDS:
        ref = restate(raw, n, scale, 1.0, kind)
        got = d.read(call_lr(d, net, fl, fr, enc, n, h, w, kind, 1.0, src_w=83), kind)
        assert_equal(got, ref, kind)
    print("%s %s: max_diff 1 px keeps %.1f %% of the pixels" % (model, rt, 100.0 * ref["valid_count"].sum() / (n * h * w)))
    # another tolerance; the optional outputs may be absent
    out = d.nan(n, 1, h, w)
    net.execute_frames_lr(fl, fr, enc, out, kind=capi.RT_DISP_PIXELS_F32, max_diff_px=3.0, batch=n, src_w=83)
    assert np.array_equal(d.get(out), restate(raw, n, scale, 3.0, capi.RT_DISP_PIXELS_F32)["out"])
    # 2 * batch > max_batch, a negative or NaN tolerance, an unknown kind or encoding, up-scaling: RtError and nothing written
    f3 = d.put(pack(images(3, 51, 83, 1), capi.RT_ENC_BGR8))
    small = d.put(pack(images(2, 20, 30, 1), capi.RT_ENC_BGR8))
    bufs = d.outputs(3, h, w, capi.RT_DISP_PIXELS_F32)
    for args, kw in (((f3, f3, capi.RT_ENC_BGR8, 3), dict(src_w=83)),
                     ((f3, f3, capi.RT_ENC_BGR8, 2), dict(src_w=83, max_diff=-1.0)),
                     ((f3, f3, capi.RT_ENC_BGR8, 2), dict(src_w=83, max_diff=float("nan"))),
                     ((f3, f3, capi.RT_ENC_BGR8, 2), dict(src_w=83, kind=3)),
                     ((f3, f3, capi.RT_ENC_BGR8, 2), dict(src_w=83, kind=-1)),
                     ((f3, f3, 7, 2), dict(src_w=83)),
                     ((small, small, capi.RT_ENC_BGR8, 2), dict(src_w=30))):
        with pytest.raises(capi.RtError) as e:
            call_lr(d, net, args[0], args[1], args[2], args[3], h, w, kw.pop("kind", capi.RT_DISP_PIXELS_F32), kw.pop("max_diff", 1.0), bufs=bufs,
                    **kw)
        got = d.read(bufs, capi.RT_DISP_PIXELS_F32)
        assert np.isnan(got["out"]).all() and np.isnan(got["right_out"]).all() and (got["mask"] == 7).all(), str(e.value)
        assert (got["valid_count"] == 12345).all(), str(e.value)
        if args[3] == 3:
            assert "6" in str(e.value) and "4" in str(e.value)          # names the engine batch it needs and max_batch
    net.destroy()


def test_execute_frames_lr_beside_execute_frames_in_graph_mode(rt):
    """a camera ring: three sets of frame, disparity and mask buffers in rotation on a stream with graph mode on, every checked call
    followed by a plain rt_net_execute_frames at half the engine batch -- two graphs on the same bindings; all equal to the direct results.
    (The emulator has no graphs: there the engine falls back to launching directly, and the rotation and the alternation still run.)"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    n, enc = 2, capi.RT_ENC_BGRA8
    if rt == "gpu":
        h, w, sh, sw, md = 129, 257, 376, 672, 16
    else:
        h, w, sh, sw, md = 25, 41, 51, 83, 8
    net = lib.create("resnet18_2D", w, h, max_batch=2 * n, weights=O.synth_weights_resnet18_2d(), max_disp=md)
    sets = [(d.put(pack(images(n, sh, sw, 40 + 2 * i), enc, PAD, i)), d.put(pack(images(n, sh, sw, 41 + 2 * i), enc, PAD, i + 7))) for i in range(3)]
    kind = capi.RT_DISP_PIXELS_F32

    def plain(i, out, stream=None):
        net.execute_frames(sets[i][0], sets[i][1], enc, out, kind=kind, batch=n, stream=stream, src_w=sw)

    direct, direct_plain = [], []
    for i in range(3):
        direct.append(d.read(call_lr(d, net, sets[i][0], sets[i][1], enc, n, h, w, kind, 1.0, src_w=sw), kind))
        out = d.nan(n, 1, h, w)
        plain(i, out)
        direct_plain.append(d.get(out))
    assert not np.isnan(direct_plain[0]).any() and not np.array_equal(direct[0]["mask"], direct[1]["mask"])
    if rt == "gpu":
        s = torch.cuda.Stream()
        stream, sync = s.cuda_stream, s.synchronize
    else:
        handle = ctypes.c_void_p()
        lib.kernels.check(lib.kernels.lib.rt_stream_create(ctypes.byref(handle)), "rt_stream_create")
        stream = handle.value
        sync = lambda: lib.kernels.check(lib.kernels.lib.rt_stream_sync(stream), "rt_stream_sync")      # noqa: E731
    net.set_graph(True)
    for call in range(9 if rt == "gpu" else 3):          # per engine batch: 1 direct, 2 capture + launch, then replays
        i = call % 3
        bufs, out = d.outputs(n, h, w, kind), d.nan(n, 1, h, w)
        if rt == "gpu":
            torch.cuda.synchronize()
        call_lr(d, net, sets[i][0], sets[i][1], enc, n, h, w, kind, 1.0, bufs=bufs, src_w=sw, stream=stream)
        plain(i, out, stream=stream)
        sync()
        assert_equal(d.read(bufs, kind), direct[i], call)
        assert np.array_equal(d.get(out), direct_plain[i]), call
    for call in range(3 if rt == "gpu" else 1):          # and on the NULL stream, synchronously
        i = (call + 1) % 3
        assert_equal(d.read(call_lr(d, net, sets[i][0], sets[i][1], enc, n, h, w, kind, 1.0, src_w=sw), kind), direct[i], call)
    net.destroy()
    if rt != "gpu":
        lib.kernels.lib.rt_stream_destroy(stream)


# ---- 5. GPU only: trained weights on the reference's sample pair against the CPU oracle ----------------------------------------------------
def oracle_two_views(h, w):
    """the CPU oracle's (2,1,h,w) output for the sample pair and for its mirrored, swapped twin (ResNet-18 2D, fp32 weights)"""
    left, right = (O.preprocess_bgr8(img[0], h, w) for img in sample_bgr())
    weights = O.read_weights(model_files.weight_file("resnet18_2D"))
    with torch.no_grad():
        a = O.resnet18_2d(torch.from_numpy(left)[None], torch.from_numpy(right)[None], weights).numpy()
        b = O.resnet18_2d(torch.from_numpy(np.ascontiguousarray(right[..., ::-1]))[None],
                          torch.from_numpy(np.ascontiguousarray(left[..., ::-1]))[None], weights).numpy()
    return np.concatenate([a, b]).reshape(2, 1, h, w).astype(np.float32)


@pytest.mark.gpu
def test_reference_sample_pair_mask_agrees_with_the_oracle():
    """ResNet-18 2D at 1025x321, fp32: the mask equals the one the restatement makes from the CPU oracle's two outputs, except where the
    oracle cannot decide within 2e-3 px (twice the 1e-3 parity budget): x - dL that close to a rounding tie, or |dL - dR(xr)| that close
    to the tolerance.  At most 2 % of the pixels may be undecided (on this pair the oracle leaves 0.50 % undecided at 1 px and 0.42 % at
    3 px: measured on the CPU, oracle alone; it finds 40.0 % and 64.7 % of the pixels consistent)."""
    lib, d = netlib("gpu"), Bufs(True)
    w, h = 1025, 321
    net = lib.create("resnet18_2D", w, h, max_batch=2, weights_path=model_files.weight_file("resnet18_2D"))
    left, right = sample_bgr()
    fl, fr = d.put(pack(left, capi.RT_ENC_BGR8)), d.put(pack(right, capi.RT_ENC_BGR8))
    oracle = oracle_two_views(h, w)
    for max_diff in (1.0, 3.0):
        got = d.read(call_lr(d, net, fl, fr, capi.RT_ENC_BGR8, 1, h, w, capi.RT_DISP_PIXELS_F32, max_diff, src_w=left.shape[2]),
                     capi.RT_DISP_PIXELS_F32)
        ref = restate(oracle, 1, w, max_diff, capi.RT_DISP_PIXELS_F32)
        skip = undecidable(oracle, 1, w, max_diff, 2e-3)
        differ = (got["mask"] != ref["mask"]) & ~skip
        print("sample pair 1025x321, max_diff %.0f px: %.2f %% consistent (oracle %.2f %%), %.3f %% undecided, %d of the rest differ"
              % (max_diff, 100.0 * got["valid_count"][0] / (h * w), 100.0 * ref["valid_count"][0] / (h * w), 100.0 * skip.mean(), differ.sum()))
        assert skip.mean() <= 0.02, skip.mean()
        assert not differ.any(), int(differ.sum())
        assert got["valid_count"][0] == (got["mask"] == 255).sum()
    net.destroy()
