"""What the camera really sends: mono8 / mono16, 8-bit Bayer and YUV 4:2:2 frames decoded on the device, in front of the frame path.

- rt_decode_frames_u8: `decode_ref` restates the definitions of include/rt_stereo.h in numpy on integer arrays (np.pad(mode="reflect") for
  the mosaic); the kernel must equal it on the raw bytes for all 8 wire encodings x 4 output encodings, on the byte path and on the dword
  path.  The restatement itself is held to its meaning by CPU-only properties: constant and ramp mosaics, pattern symmetries, all 2^24
  (Y, U, V) triples against the BT.601 formula in floating point, all 65536 mono16 values against rint.  OpenCV is not the target and
  was never compared with.
- rt_net_execute_frames_camera: one decode launch in front of rt_net_execute_frames_filtered, bit-equal to the two calls made by hand.
CPU tier: the same sources on the SIMT emulator; GPU tier (-m gpu): the MI355X, the reference's sample pair and trained weights."""
import ctypes

import numpy as np
import pytest
import torch

from redtail_amd import capi, model_files
from test_camera_frames import ENCODINGS, PAD, netlib, pack, rt, sample_bgr  # noqa: F401  (rt: the emu / gpu fixture)
from test_frames_any_size import NETS, NET_IDS
from test_lr_consistency import Bufs, make_net
from test_points import SENTINEL, bufs_3d, camera, compare_3d, read_points
from test_rectify import raw_pair, rectify_by_hand, rig
from test_speckle import call_filtered

f32 = np.float32
PIXELS, U16 = capi.RT_DISP_PIXELS_F32, capi.RT_DISP_KITTI_U16
M_F32, MM_U16 = capi.RT_DEPTH_M_F32, capi.RT_DEPTH_MM_U16
CV, DOWN = capi.RT_RESIZE_CV_AREA, capi.RT_RESIZE_AREA_DOWN
INF = float("inf")
ALL = ("depth", "points", "compact")
ENC_IDS = ["bgr8", "rgb8", "bgra8", "rgba8"]
BAYER = {capi.RT_WIRE_BAYER_RGGB8: "rggb", capi.RT_WIRE_BAYER_BGGR8: "bggr", capi.RT_WIRE_BAYER_GBRG8: "gbrg", capi.RT_WIRE_BAYER_GRBG8: "grbg"}
YUV = (capi.RT_WIRE_YUV422, capi.RT_WIRE_YUV422_YUY2)
WIRES = [capi.RT_WIRE_MONO8, capi.RT_WIRE_MONO16, *BAYER, *YUV]
WIRE_IDS = ["mono8", "mono16", "bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8", "yuv422", "yuv422_yuy2"]


# ---- the definition restated in numpy: (n, h, row bytes) wire rows -> (n, h, w, 3) R, G, B as integers ---------------------------------------
def mono16_ref(v16):
    v16 = np.asarray(v16, np.int64)
    return np.minimum(255, (v16 + 127 + ((v16 >> 8) & 1)) >> 8)


def bayer_ref(m, pattern):
    """bilinear demosaicing of the mosaic m (n, h, w) whose top-left 2 x 2 is `pattern`, row-major"""
    n, h, w = m.shape
    p = np.pad(m.astype(np.int64), ((0, 0), (1, 1), (1, 1)), mode="reflect")
    at = lambda dy, dx: p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    here = at(0, 0)
    hs, vs = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0)
    cross, diag = (hs + vs + 2) >> 2, (at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1) + 2) >> 2
    hav, vav = (hs + 1) >> 1, (vs + 1) >> 1
    y, x = np.indices((h, w))
    colour = np.array(list(pattern))
    site, beside = colour[2 * (y & 1) + (x & 1)], colour[2 * (y & 1) + ((x & 1) ^ 1)]
    out = np.empty((n, h, w, 3), np.int64)
    for c, (name, other) in enumerate((("r", "b"), ("g", None), ("b", "r"))):
        if name == "g":
            out[..., c] = np.where(site == "g", here, cross)
        else:
            out[..., c] = np.where(site == name, here, np.where(site == other, diag, np.where(beside == name, hav, vav)))
    return out


def yuv_ref(Y, U, V):
    CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527
    Y, U, V = (np.asarray(a, np.int64) for a in (Y, U, V))
    y = np.maximum(0, Y - 16) * CY + (1 << 19)
    r = (y + CVR * (V - 128)) >> 20
    g = (y + CVG * (V - 128) + CUG * (U - 128)) >> 20
    b = (y + CUB * (U - 128)) >> 20
    assert max(np.abs(t).max() for t in (y + CVR * (V - 128), y + CVG * (V - 128) + CUG * (U - 128), y + CUB * (U - 128))) < 2 ** 31
    return np.stack([np.clip(t, 0, 255) for t in (r, g, b)], axis=-1)


def decode_ref(rows, w, wire):
    n, h, _ = rows.shape
    if wire == capi.RT_WIRE_MONO8:
        v = rows[:, :, :w].astype(np.int64)
        return np.stack([v, v, v], axis=-1)
    if wire == capi.RT_WIRE_MONO16:
        b = rows[:, :, :2 * w].astype(np.int64)
        v = mono16_ref(b[:, :, 0::2] | (b[:, :, 1::2] << 8))
        return np.stack([v, v, v], axis=-1)
    if wire in BAYER:
        return bayer_ref(rows[:, :, :w], BAYER[wire])
    q = rows[:, :, :2 * w].reshape(n, h, w // 2, 4).astype(np.int64)
    u, y0, v, y1 = (q[..., i] for i in ((0, 1, 2, 3) if wire == capi.RT_WIRE_YUV422 else (1, 0, 3, 2)))
    return np.stack([yuv_ref(y0, u, v), yuv_ref(y1, u, v)], axis=3).reshape(n, h, w, 3)


def encode(rgb, enc):
    """(n, h, w, 3) R, G, B -> (n, h, w * bpp) bytes of an RT_ENC_* frame, alpha 255"""
    n, h, w, _ = rgb.shape
    px = rgb if enc in (capi.RT_ENC_RGB8, capi.RT_ENC_RGBA8) else rgb[..., ::-1]
    if capi.ENC_BYTES[enc] == 4:
        px = np.concatenate([px, np.full((n, h, w, 1), 255, px.dtype)], axis=3)
    return px.astype(np.uint8).reshape(n, h, -1)


def wire_rows(n, h, w, wire, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w * capi.WIRE_BYTES[wire]), dtype=np.uint8)


# ---- buffers at a chosen base alignment -----------------------------------------------------------------------------------------------------
SLACK = 16


class Placed:
    """n frames of h rows, `step` bytes apart, in a flat device buffer whose first frame byte lies `misalign` bytes past a 4-byte boundary;
    the buffer starts as `fill` (an array of its size, or a byte) and keeps SLACK bytes or more on either side of the frames"""

    def __init__(self, d, n, h, row_bytes, step, misalign, fill):
        self.d, self.shape, self.row_bytes = d, (n, h, step), row_bytes
        self.size = n * h * step + 2 * SLACK
        host = np.full(self.size, fill, np.uint8) if np.isscalar(fill) else np.asarray(fill, np.uint8)[:self.size].copy()
        self.buf = d.put(host)
        self.off = SLACK + (misalign - (capi._ptr(self.buf) + SLACK)) % 4
        self.ptr = capi._ptr(self.buf) + self.off
        assert self.ptr % 4 == misalign and self.off + n * h * step <= self.size

    def window(self, host):
        n, h, step = self.shape
        return host[self.off:self.off + n * h * step].reshape(n, h, step)

    def put_rows(self, rows):
        host = np.array(self.d.get(self.buf))
        self.window(host)[:, :, :self.row_bytes] = rows
        self.buf[...] = self.d.put(host)
        return self

    def get(self):
        return np.array(self.d.get(self.buf))

    def expect(self, rows, fill):
        want = np.full(self.size, fill, np.uint8)
        self.window(want)[:, :, :self.row_bytes] = rows
        return want


def round4(v):
    return (v + 3) // 4 * 4


# form -> (source step, destination step, misalignment of every base) from the row sizes
FORMS = {"dense": lambda s, t: (s, t, 0), "step+3": lambda s, t: (s + 3, t + 3, 0), "odd-base": lambda s, t: (s, t, 1),
         "aligned": lambda s, t: (round4(s) + 4, round4(t) + 8, 0)}


def new_stream(rt_name, k):
    if rt_name == "gpu":
        s = torch.cuda.Stream()
        return s.cuda_stream, s.synchronize, lambda: None
    handle = ctypes.c_void_p()
    k.check(k.lib.rt_stream_create(ctypes.byref(handle)), "rt_stream_create")
    return handle.value, lambda: k.check(k.lib.rt_stream_sync(handle.value), "rt_stream_sync"), lambda: k.lib.rt_stream_destroy(handle.value)


# ---- 1. the op against its restatement, bit for bit ------------------------------------------------------------------------------------------
SHAPES = [(2, 2), (5, 6), (7, 10), (9, 263)]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=["2x2", "6x5", "10x7", "263x9"])
@pytest.mark.parametrize("wire", WIRES, ids=WIRE_IDS)
def test_bit_equal_to_restatement(backend, wire, shape, form):
    """All four output encodings of one wire encoding, shape and memory form; batch 2, left and right differ.  2 x 2 is the Bayer minimum
    (every pixel a border pixel); 263 columns (262 for YUV, which needs an even width) are wider than the 256 a block spans and no
    multiple of the 4-pixel run of a lane; 5, 7 and 9 rows are no multiple of the rows of a block.  `odd-base` and `step+3` take the byte
    path, `aligned` the dword path, `dense` whichever the row size gives.  Random bytes fill the source's padding; the sentinel in the
    destination's padding, in front of the first frame and behind the last one must survive.  A second run on a stream of its own agrees."""
    d, k = Bufs(backend.name == "gpu"), backend.klib
    h, w = shape
    if wire in YUV:
        w -= w % 2
    n, wb = 2, capi.WIRE_BYTES[wire]
    rows = [wire_rows(n, h, w, wire, seed=11 * wire + side) for side in (0, 1)]
    rgb = [decode_ref(r, w, wire) for r in rows]
    assert rgb[0].tobytes() != rgb[1].tobytes()
    stream, sync, done = new_stream(backend.name, k)
    for enc in ENCODINGS:
        bpp = capi.ENC_BYTES[enc]
        step, dstep, mis = FORMS[form](w * wb, w * bpp)
        noise = np.random.default_rng(wire + enc).integers(0, 256, n * h * step + 2 * SLACK + 8, dtype=np.uint8)
        src = [Placed(d, n, h, w * wb, step, mis, noise).put_rows(r) for r in rows]
        want = [encode(c, enc) for c in rgb]
        for run in (0, 1):
            dst = [Placed(d, n, h, w * bpp, dstep, mis, SENTINEL) for _ in (0, 1)]
            k.decode_frames_u8(src[0].ptr, src[1].ptr, h, w, step, wire, dst[0].ptr, dst[1].ptr, dstep, enc, n, stream=stream if run else None)
            sync()
            for side in (0, 1):
                got, ref = dst[side].get(), dst[side].expect(want[side], SENTINEL)
                assert np.array_equal(got, ref), (ENC_IDS[enc], run, side, int((got != ref).sum()), np.flatnonzero(got != ref)[:8])
    done()


# ---- 2. the restatement held to its meaning (CPU only) ----------------------------------------------------------------------------------------
def mosaic(rgb, pattern):
    """what a sensor with this colour filter array records of an (n, h, w, 3) R, G, B picture"""
    n, h, w, _ = rgb.shape
    y, x = np.indices((h, w))
    channel = np.array(["rgb".index(c) for c in pattern])[2 * (y & 1) + (x & 1)]
    return np.take_along_axis(rgb, np.broadcast_to(channel[None, :, :, None], (n, h, w, 1)), axis=3)[..., 0]


@pytest.mark.parametrize("pattern", list(BAYER.values()))
def test_bayer_constant_colour_and_ramps(pattern):
    """a constant colour comes back at every pixel, border included; a per-channel integer ramp a x + b y + c comes back exactly away from
    the border (the neighbours of a pixel average to the pixel: the sums are whole multiples of their divisor, nothing is rounded)"""
    for h, w in ((2, 2), (5, 6), (9, 13)):
        flat = np.broadcast_to(np.array([200, 17, 90]), (1, h, w, 3))
        assert np.array_equal(bayer_ref(mosaic(flat, pattern), pattern), flat), (pattern, h, w)
    h, w = 11, 14
    y, x = np.indices((h, w))
    ramp = np.stack([3 * x + 2 * y + 5, 4 * x + 7 * y + 1, 9 * x + y + 30], axis=-1)[None]
    assert ramp.max() <= 255
    got = bayer_ref(mosaic(ramp, pattern), pattern)
    assert np.array_equal(got[:, 1:-1, 1:-1], ramp[:, 1:-1, 1:-1]), pattern


def test_bayer_patterns_are_one_formula():
    """bggr is rggb with R and B exchanged, gbrg is grbg likewise; a mosaic shifted by one column turns rggb into grbg on the interior"""
    m = np.random.default_rng(3).integers(0, 256, (2, 9, 12))
    assert np.array_equal(bayer_ref(m, "bggr"), bayer_ref(m, "rggb")[..., ::-1])
    assert np.array_equal(bayer_ref(m, "gbrg"), bayer_ref(m, "grbg")[..., ::-1])
    assert np.array_equal(bayer_ref(m[:, :, 1:], "grbg")[:, :, 1:-1], bayer_ref(m, "rggb")[:, :, 2:-1])
    assert np.array_equal(bayer_ref(m[:, 1:, :], "gbrg")[:, 1:-1], bayer_ref(m, "rggb")[:, 2:-1])


def test_yuv_all_triples_against_the_float_formula():
    """every (Y, U, V): each channel within 1 level of clamp(floor(1.164 (Y - 16)+ + k_v (V - 128) + k_u (U - 128) + 0.5)) with the 3-digit
    BT.601 coefficients -- the integer coefficients are those rounded to 2^-20 from more digits, so the two sums differ by less than one
    level before the floor -- and differ for under 0.2 % of the triples per channel.  Grey (U = V = 128) is grey, 16 -> 0, 235 -> 255."""
    u, v = (a.reshape(-1) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    k = np.array([[0.0, 1.596], [-0.391, -0.813], [2.018, 0.0]])          # (k_u, k_v) of R, G, B
    differ = np.zeros(3)
    for Y in range(256):
        got = yuv_ref(np.full(u.shape, Y), u, v)
        for c in range(3):
            want = np.clip(np.floor(1.164 * max(0, Y - 16) + k[c, 1] * (v - 128) + k[c, 0] * (u - 128) + 0.5), 0, 255)
            diff = np.abs(got[:, c] - want)
            assert diff.max() <= 1, (Y, c, diff.max())
            differ[c] += (diff != 0).sum()
    print("share of triples that differ from the float formula, R G B:", differ / 2 ** 24)
    assert (differ / 2 ** 24 < 0.002).all(), differ / 2 ** 24
    grey = yuv_ref(np.arange(256), np.full(256, 128), np.full(256, 128))
    assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 0] == grey[:, 2]).all()
    assert grey[16].tolist() == [0, 0, 0] and grey[235].tolist() == [255, 255, 255] and (np.diff(grey[:, 0]) >= 0).all()


def test_uyvy_and_yuyv_of_the_same_samples_decode_alike():
    q = np.random.default_rng(4).integers(0, 256, (2, 5, 7, 4), dtype=np.uint8)        # U Y0 V Y1
    uyvy, yuyv = q.reshape(2, 5, 28), q[..., [1, 0, 3, 2]].reshape(2, 5, 28)
    a, b = decode_ref(uyvy, 14, capi.RT_WIRE_YUV422), decode_ref(yuyv, 14, capi.RT_WIRE_YUV422_YUY2)
    assert np.array_equal(a, b)
    q[..., 3] = q[..., 1]                                  # the same Y twice: a pair shares U and V, so its two pixels are one colour
    a = decode_ref(q.reshape(2, 5, 28), 14, capi.RT_WIRE_YUV422)
    assert np.array_equal(a[:, :, 0::2], a[:, :, 1::2])


def test_mono16_all_values_round_to_nearest_even():
    v = np.arange(65536)
    assert np.array_equal(mono16_ref(v), np.clip(np.rint(v / 256.0), 0, 255).astype(np.int64))
    rows = v.astype("<u2").view(np.uint8).reshape(1, 256, 512)
    assert np.array_equal(decode_ref(rows, 256, capi.RT_WIRE_MONO16)[0, :, :, 1].reshape(-1), mono16_ref(v))


# ---- 3. refusals write nothing ----------------------------------------------------------------------------------------------------------------
def test_op_refusals(backend):
    d, k = Bufs(backend.name == "gpu"), backend.klib
    h, w, bpp = 6, 8, 4
    src = [d.put(wire_rows(1, h, w, capi.RT_WIRE_YUV422, s)) for s in (1, 2)]
    out = [d.full((1, h, w * bpp), np.uint8, SENTINEL) for _ in (0, 1)]
    same = d.full((1, h, w * bpp), np.uint8, SENTINEL)

    def go(**kw):
        a = dict(left=src[0], right=src[1], h=h, w=w, step=2 * w, wire=capi.RT_WIRE_YUV422, dl=out[0], dr=out[1], dstep=w * bpp, enc=capi.RT_ENC_BGRA8,
                 n=1)
        a.update(kw)
        k.decode_frames_u8(a["left"], a["right"], a["h"], a["w"], a["step"], a["wire"], a["dl"], a["dr"], a["dstep"], a["enc"], a["n"])

    bad = [dict(left=None), dict(right=None), dict(dl=None), dict(dr=None)]
    bad += [dict(wire=v) for v in (-1, 0, 1, 2, 3, 4, 7, 9, 15, 24)]
    bad += [dict(enc=v) for v in (-1, 4, 16, 22)]
    bad += [dict(h=0), dict(w=0), dict(n=0), dict(h=-3), dict(n=32768), dict(h=4 * 65535 + 1), dict(w=(1 << 24) + 2, step=1 << 30, dstep=1 << 30)]
    bad += [dict(wire=b, h=1) for b in BAYER] + [dict(wire=capi.RT_WIRE_BAYER_GBRG8, w=1)]
    bad += [dict(w=7, wire=y) for y in YUV]
    bad += [dict(step=2 * w - 1), dict(step=w - 1, wire=capi.RT_WIRE_MONO8), dict(step=2 * w - 1, wire=capi.RT_WIRE_MONO16), dict(step=0), dict(step=-16)]
    bad += [dict(dstep=w * bpp - 1), dict(dstep=w * 3 - 1, enc=capi.RT_ENC_RGB8), dict(dstep=0)]
    bad += [dict(left=same, dl=same), dict(right=same, dr=same), dict(left=same, dr=same), dict(dl=same, dr=same)]
    for kw in bad:
        with pytest.raises(capi.RtError):
            go(**kw)
        assert all((d.get(o) == SENTINEL).all() for o in out + [same]), kw
    go()                                                   # and next to them it works
    assert not any((d.get(o) == SENTINEL).all() for o in out)
    go(wire=capi.RT_WIRE_MONO8, w=7, step=2 * w)           # an odd width is legal for mono and Bayer
    go(wire=capi.RT_WIRE_BAYER_BGGR8, w=7, h=3, step=2 * w)


def camera_outputs(d, n, sh, sw, bpp, pad=PAD):
    b = bufs_3d(d, n, sh, sw, True, ALL, True)
    for key in ("left_rect", "right_rect", "left_color", "right_color"):
        b[key] = d.full((n, sh, sw * bpp + pad), np.uint8, SENTINEL)
    return b


FRAMES = ("left_rect", "right_rect", "left_color", "right_color")


def camera_untouched(d, b):
    g = read_points(d, {key: v for key, v in b.items() if key not in FRAMES}, PIXELS, M_F32)
    return (np.isnan(g["disp"]).all() and (g["mask"] == 7).all() and (g["valid_count"] == 12345).all() and
            (g["depth"] == f32(1e30).view(np.uint32)).all() and (g["points"].view(np.uint8) == SENTINEL).all() and
            (g["compact"].view(np.uint8) == SENTINEL).all() and (g["count"] == 12345).all() and all((d.get(b[key]) == SENTINEL).all() for key in FRAMES))


def call_camera(net, fl, fr, wire, enc, cam, b, n, resize, max_diff, speckle, zmin=0.0, zmax=INF, depth_kind=M_F32, disp_kind=PIXELS, **kw):
    net.execute_frames_camera(fl, fr, wire, enc, speckle_size=None if speckle is None else speckle[0],
                              speckle_range=1.0 if speckle is None else speckle[1], camera=cam, disp=b["disp"], kind=disp_kind, resize=resize,
                              max_diff_px=max_diff, mask=b["mask"], valid_count=b["valid_count"], min_depth=zmin, max_depth=zmax, depth=b["depth"],
                              depth_kind=depth_kind, points=b["points"], points_compact=b["compact"], count=b["count"], batch=n, **kw)


def test_net_refusals_write_nothing(rt):
    """what only the new struct can get wrong, and refusals of the wrapped calls reached through the new entry: an error, and every
    sentinel-filled output -- the caller's decoded and rectified frames among them -- untouched"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    net, h, w, scale = make_net(lib, "resnet18_2D")
    n, enc, bpp, sh, sw = 1, capi.RT_ENC_BGRA8, 4, 30, 36
    wire = capi.RT_WIRE_BAYER_GRBG8
    cl, cr = rig(k, sh, sw, fx=40.0)
    fl, fr = (d.put(wire_rows(n, sh, sw, wire, s)) for s in (5, 6))
    yl, yr = (d.put(wire_rows(n, sh, sw - 1, capi.RT_WIRE_YUV422, s)) for s in (7, 8))            # an odd width
    big_l, big_r = (d.put(wire_rows(5, sh, sw, wire, s)) for s in (9, 10))
    small = d.put(wire_rows(n, 20, 30, wire, 11))          # the down-only filter refuses it: both axes would grow
    wide = d.put(wire_rows(n, 4, 250, wire, 12))           # 250 / 41 > 6
    cam = camera(fx=30.0, fy=31.0, cx=18.0, cy=15.0, baseline=0.1)
    b = camera_outputs(d, n, sh, sw, bpp)
    nan = float("nan")
    bad = [dict(decode_struct_bytes=ctypes.sizeof(capi.DecodeCall) - 8), dict(decode_struct_bytes=0)]
    bad += [dict(wire=v) for v in (-1, 0, 3, 15, 24)]
    bad += [dict(enc=v) for v in (-1, 4, 16, wire)]
    bad += [dict(right_color=None), dict(left_color=None), dict(color_step=sw * bpp - 1), dict(left_color=None, right_color=None, color_step=sw * bpp),
            dict(left_color=fl), dict(right_color=fr), dict(left_color=b["left_rect"]), dict(right_color=b["right_rect"]),
            dict(left_color=b["right_color"]), dict(src_step=sw - 1), dict(fl=yl, fr=yr, wire=capi.RT_WIRE_YUV422, src_w=sw - 1),
            dict(resize=DOWN, fl=small, fr=small, src_w=30), dict(fl=wide, fr=wide, src_w=250), dict(src_w=0), dict(batch=0),
            dict(batch=3, fl=big_l, fr=big_r)]
    bad += [dict(rect_struct_bytes=0), dict(right_rect=None), dict(rect_step=sw * bpp - 1), dict(geometry=capi.RT_GEOM_NET),
            dict(struct_bytes=ctypes.sizeof(capi.FrameCall) - 8), dict(depth_struct_bytes=0), dict(speckle_struct_bytes=0), dict(speckle=(-1, 1.0)),
            dict(resize=2), dict(disp_kind=3), dict(disp_kind=capi.RT_DISP_NET), dict(depth_kind=2), dict(max_diff=nan), dict(cam=camera(fx=0.0)),
            dict(zmin=2.0, zmax=1.0)]
    for kw in bad:
        kw = dict(kw)
        a = dict(resize=CV, max_diff=1.5, cam=cam, fl=fl, fr=fr, batch=n, wire=wire, enc=enc, speckle=(2, 1.0), src_w=sw)
        for key in list(a):
            if key in kw:
                a[key] = kw.pop(key)
        frames = {key: kw.pop(key, b[key]) for key in FRAMES}
        with pytest.raises(capi.RtError) as e:
            call_camera(net, a["fl"], a["fr"], a["wire"], a["enc"], a["cam"], b, a["batch"], a["resize"], a["max_diff"], a["speckle"],
                        src_w=a["src_w"], rect_left=cl, rect_right=cr, **frames, **kw)
        assert "rt_net_execute_frames_camera" in str(e.value), str(e.value)
        assert camera_untouched(d, b), (kw, a["wire"], a["enc"])
    call_camera(net, fl, fr, wire, enc, cam, b, n, CV, 1.5, (2, 1.0), src_w=sw, rect_left=cl, rect_right=cr, **{key: b[key] for key in FRAMES})
    assert not camera_untouched(d, b)                      # and the valid call works
    assert not (d.get(b["left_color"])[:, :, :sw * bpp] == SENTINEL).all() and (d.get(b["left_color"])[:, :, sw * bpp:] == SENTINEL).all()
    net.destroy()


# ---- 4. the net call is its composition -------------------------------------------------------------------------------------------------------
def decode_by_hand(k, d, fl, fr, sh, sw, wire, enc, n, pad=0):
    bpp = capi.ENC_BYTES[enc]
    out = d.full((n, sh, sw * bpp + pad), np.uint8, SENTINEL), d.full((n, sh, sw * bpp + pad), np.uint8, SENTINEL)
    k.decode_frames_u8(fl, fr, sh, sw, fl.shape[2], wire, *out, sw * bpp + pad, enc, n)
    return out


@pytest.mark.parametrize("model,flags", NETS, ids=NET_IDS)
def test_execute_frames_camera_equals_the_two_calls_by_hand(rt, model, flags):
    """rt_net_execute_frames_camera against rt_decode_frames_u8 into dense buffers followed by rt_net_execute_frames_filtered on them, bit
    for bit.  Everything on, from bayer_grbg8 with padded wire rows: rect, check, speckle and out (16-bit disparity, mask, count, depth,
    organised and compact cloud), into the caller's padded colour and rectified buffers, which then hold what the ops write.  Everything
    off, from yuv422_yuy2: a larger frame into the net's own colour buffers, with the disparity alone.  (An engine pass on the emulator takes seconds, so each camera call has one counterpart by hand.)"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    net, h, w, scale = make_net(lib, model, flags)
    n = 2 if flags else 1
    # everything on
    sh, sw, wire, enc, bpp = 30, 36, capi.RT_WIRE_BAYER_GRBG8, capi.RT_ENC_RGBA8, 4
    cl, cr = rig(k, sh, sw, fx=40.0)
    cam = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)
    rows = [np.pad(wire_rows(n, sh, sw, wire, s), ((0, 0), (0, 0), (0, 5)), constant_values=0x5A) for s in (20, 21)]
    fl, fr = d.put(rows[0]), d.put(rows[1])
    dl, dr = decode_by_hand(k, d, fl, fr, sh, sw, wire, enc, n)
    assert np.array_equal(d.get(dl), encode(decode_ref(rows[0], sw, wire), enc))
    speckle = (2, 1.0)
    ref = bufs_3d(d, n, sh, sw, True, ALL, True, MM_U16, U16)
    call_filtered(net, dl, dr, enc, cam, ref, n, CV, 1.5, speckle, 0.05, 1.0, MM_U16, U16, src_w=sw, rect_left=cl, rect_right=cr)
    ref = read_points(d, ref, U16, MM_U16)
    assert 0 < ref["count"].sum() <= n * sh * sw
    b = camera_outputs(d, n, sh, sw, bpp)
    b.update(bufs_3d(d, n, sh, sw, True, ALL, True, MM_U16, U16))
    frames = {key: b.pop(key) for key in FRAMES}
    call_camera(net, fl, fr, wire, enc, cam, b, n, CV, 1.5, speckle, 0.05, 1.0, MM_U16, U16, src_w=sw, rect_left=cl, rect_right=cr, **frames)
    compare_3d(read_points(d, b, U16, MM_U16), ref, n, sh * sw, "all on")
    want = decode_by_hand(k, d, fl, fr, sh, sw, wire, enc, n, PAD)
    rect = rectify_by_hand(k, d, dl, dr, sh, sw, enc, cl, cr, n, PAD)
    for key, buf in zip(FRAMES, rect + want):
        assert np.array_equal(d.get(frames[key]), d.get(buf)), key
        assert (d.get(frames[key])[:, :, sw * bpp:] == SENTINEL).all() and not (d.get(frames[key]) == SENTINEL).all()
    # everything off, a larger frame, the net's own buffers
    sh, sw, wire, enc = 51, 84, capi.RT_WIRE_YUV422_YUY2, capi.RT_ENC_BGR8
    rows = [wire_rows(n, sh, sw, wire, s) for s in (22, 23)]
    fl, fr = d.put(rows[0]), d.put(rows[1])
    dl, dr = decode_by_hand(k, d, fl, fr, sh, sw, wire, enc, n)
    old, new = d.nan(n, 1, sh, sw), d.nan(n, 1, sh, sw)
    net.execute_frames_filtered(dl, dr, enc, disp=old, resize=DOWN, batch=n, src_w=sw, no_depth_call=True)
    net.execute_frames_camera(fl, fr, wire, enc, disp=new, resize=DOWN, batch=n, no_depth_call=True)
    got, ref = d.get(new), d.get(old)
    assert np.isfinite(ref).all() and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    net.destroy()


def test_no_decode_is_the_wrapped_call(rt):
    """decode == NULL: rt_net_execute_frames_filtered on the same arguments -- the outputs, and the error texts under its own names"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    net, h, w, scale = make_net(lib, "resnet18_2D")
    n, enc, sh, sw = 1, capi.RT_ENC_BGRA8, 30, 36
    cl, cr = rig(k, sh, sw, fx=40.0)
    cam = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)
    fl, fr = (d.put(f) for f in raw_pair(n, sh, sw, enc, PAD, seed=30))
    old, new = bufs_3d(d, n, sh, sw, True, ALL, True), bufs_3d(d, n, sh, sw, True, ALL, True)
    call_filtered(net, fl, fr, enc, cam, old, n, CV, -1.0, (2, 1.0), src_w=sw, rect_left=cl, rect_right=cr)
    call_camera(net, fl, fr, None, enc, cam, new, n, CV, -1.0, (2, 1.0), src_w=sw, rect_left=cl, rect_right=cr)
    compare_3d(read_points(d, new, PIXELS, M_F32), read_points(d, old, PIXELS, M_F32), n, sh * sw, "decode == NULL")
    cases = [dict(speckle=(2, 1.0), rect_left=cl, rect_right=cr, max_diff=float("nan")), dict(speckle=None, rect_left=cl, rect_right=cr, rect_step=5),
             dict(speckle=None, depth_kind=2), dict(speckle=None, no_depth_call=True, resize=7), dict(speckle=(2, 1.0), geometry=capi.RT_GEOM_NET), dict(speckle=None, disp_kind=capi.RT_DISP_NET)]
    for kw in cases:
        texts = []
        for call in (call_filtered, call_camera):
            a = dict(kw)
            args = [a.pop("enc", enc), cam, new, n, a.pop("resize", CV), a.pop("max_diff", 1.5), a.pop("speckle")]
            with pytest.raises((capi.RtError, ValueError)) as e:
                call(net, fl, fr, *(([None] if call is call_camera else []) + args), src_w=sw, **a)
            texts.append(str(e.value).replace("rt_net_execute_frames_camera failed", "rt_net_execute_frames_filtered failed"))
        assert texts[0] == texts[1] and "frames_camera" not in texts[1], texts
    net.destroy()


def test_camera_in_graph_mode_with_rotating_buffers(rt):
    """a camera ring: sets of wire and output buffers in rotation on a stream with graph mode on, then on the NULL stream: every call equal
    to the decode and the wrapped call made by hand.  Then a larger frame: the net's own colour buffers regrow.  (The emulator has no
    graphs: there the engine launches directly, and a shorter rotation still runs -- an engine pass takes seconds on it.)"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    net, h, w, scale = make_net(lib, "resnet18_2D")
    n, enc, sh, sw, wire = 1, capi.RT_ENC_BGR8, 30, 36, capi.RT_WIRE_BAYER_RGGB8
    cam = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)
    count = 3 if rt == "gpu" else 2
    sets = [(d.put(wire_rows(n, sh, sw, wire, 40 + i)), d.put(wire_rows(n, sh, sw, wire, 50 + i))) for i in range(count)]

    def go(i, b, stream=None):
        call_camera(net, sets[i][0], sets[i][1], wire, enc, cam, b, n, CV, -1.0, None, 0.05, 1.0, stream=stream)

    direct = []
    for i in range(count):
        dl, dr = decode_by_hand(k, d, sets[i][0], sets[i][1], sh, sw, wire, enc, n)
        b = bufs_3d(d, n, sh, sw, True, ALL, False)
        call_filtered(net, dl, dr, enc, cam, b, n, CV, -1.0, None, 0.05, 1.0, src_w=sw)
        direct.append(read_points(d, b, PIXELS, M_F32))
    assert direct[0]["points"].tobytes() != direct[1]["points"].tobytes()
    stream, sync, done = new_stream(rt, k)
    net.set_graph(True)
    for call in range(7 if rt == "gpu" else 2):            # 1: direct, 2: capture + launch, then replays, whatever pointers rotate in
        i = call % count
        b = bufs_3d(d, n, sh, sw, True, ALL, False)
        if rt == "gpu":
            torch.cuda.synchronize()
        go(i, b, stream=stream)
        sync()
        compare_3d(read_points(d, b, PIXELS, M_F32), direct[i], n, sh * sw, ("graph", call))
    b = bufs_3d(d, n, sh, sw, True, ALL, False)
    go(1, b)                                               # and on the NULL stream, synchronously
    compare_3d(read_points(d, b, PIXELS, M_F32), direct[1], n, sh * sw, "null stream")
    # a larger frame follows: the net's own colour buffers, made for 36 x 30 above, regrow
    sh, sw = 51, 84
    fl, fr = (d.put(wire_rows(n, sh, sw, wire, s)) for s in (60, 61))
    dl, dr = decode_by_hand(k, d, fl, fr, sh, sw, wire, enc, n)
    old, new = d.nan(n, 1, sh, sw), d.nan(n, 1, sh, sw)
    net.execute_frames_filtered(dl, dr, enc, disp=old, batch=n, src_w=sw, no_depth_call=True)
    net.execute_frames_camera(fl, fr, wire, enc, disp=new, batch=n, no_depth_call=True)
    assert np.isfinite(d.get(old)).all() and np.array_equal(d.get(new).view(np.uint32), d.get(old).view(np.uint32))
    net.destroy()
    done()


# ---- 5. GPU only: the reference's sample pair and trained weights ------------------------------------------------------------------------------
def to_uyvy(rgb):
    """(n, h, w, 3) R, G, B -> UYVY rows: BT.601 limited range in floating point, chroma averaged over each pixel pair"""
    r, g, b = (rgb[..., c].astype(np.float64) for c in range(3))
    y = 16 + 0.257 * r + 0.504 * g + 0.098 * b
    u = (128 - 0.148 * r - 0.291 * g + 0.439 * b).reshape(*r.shape[:2], -1, 2).mean(axis=3)
    v = (128 + 0.439 * r - 0.368 * g - 0.071 * b).reshape(*r.shape[:2], -1, 2).mean(axis=3)
    q = np.stack([u, y[:, :, 0::2], v, y[:, :, 1::2]], axis=3)
    return np.clip(np.rint(q), 0, 255).astype(np.uint8).reshape(rgb.shape[0], rgb.shape[1], -1)


@pytest.mark.gpu
def test_reference_sample_pair_as_mono_bayer_and_yuv():
    """ResNet-18 2D 1257 x 369 fp32, trained weights, the reference's 1242 x 375 pair.  As mono8 (a grey copy): the disparity equals, bit
    for bit, that of the same grey pixels sent as bgr8.  Mosaiced to bayer_rggb8 and sub-sampled to yuv422 by numpy: the camera call equals
    the two calls by hand.  The mean absolute difference of each disparity from that of the original bgr8 pair is printed, not asserted
    (tools/time_decode.py records the same figures in profiles/decode.json): nobody has measured what demosaicing costs this network, so
    there is nothing to take a bound from."""
    lib, d = netlib("gpu"), Bufs(True)
    k = lib.kernels
    w, h = 1257, 369
    net = lib.create("resnet18_2D", w, h, max_batch=1, weights_path=model_files.weight_file("resnet18_2D"))
    left, right = sample_bgr()
    sh, sw = left.shape[1:3]
    enc = capi.RT_ENC_BGR8

    def disparity(fl, fr, wire=None):
        out = d.nan(1, 1, sh, sw)
        net.execute_frames_camera(fl, fr, wire, enc, disp=out, batch=1, no_depth_call=True, src_w=sw)
        return d.get(out)

    original = disparity(d.put(pack(left, enc)), d.put(pack(right, enc)))
    grey = [np.rint(0.114 * f[..., 0] + 0.587 * f[..., 1] + 0.299 * f[..., 2]).astype(np.uint8) for f in (left, right)]
    as_bgr = [d.put(pack(np.repeat(g[..., None], 3, axis=3), enc)) for g in grey]
    cases = {"mono8": (capi.RT_WIRE_MONO8, grey), "bayer_rggb8": (capi.RT_WIRE_BAYER_RGGB8, [mosaic(f[..., ::-1], "rggb").astype(np.uint8) for f in (left, right)]),
             "yuv422": (capi.RT_WIRE_YUV422, [to_uyvy(f[..., ::-1]) for f in (left, right)])}
    record = {}
    for name, (wire, rows) in cases.items():
        fl, fr = (d.put(r) for r in rows)
        got = disparity(fl, fr, wire)
        dl, dr = decode_by_hand(k, d, fl, fr, sh, sw, wire, enc, 1)
        assert np.array_equal(got.view(np.uint32), disparity(dl, dr).view(np.uint32)), name
        if name == "mono8":
            assert np.array_equal(got.view(np.uint32), disparity(*as_bgr).view(np.uint32))
        assert np.isfinite(got).all()
        record[name] = float(np.abs(got - original).mean())
        print("%s: mean |disparity - disparity of the bgr8 pair| = %.4f px" % (name, record[name]))
    assert record["mono8"] > 0
    net.destroy()
