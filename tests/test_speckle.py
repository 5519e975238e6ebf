"""Speckle filter of the camera-frame path: stereo_image_proc's speckle_size / speckle_range, cv::filterSpeckles, on the device.

- rt_disparity_speckle: connected components (4-neighbours, |d(p) - d(q)| <= max_diff in fp32) of the live pixels; those of at most
  max_size pixels are removed.  `restate` below says the same with numpy float32 edge lists, scipy's connected_components and
  np.bincount -- another algorithm than the kernels' union-find -- and every op-level case is bit-exact against it: no tolerance anywhere.
  The kernels label 32 x 32 tiles (TILE below) in LDS and merge the tile borders in global memory, so the patterns sit astride those
  borders: 70 x 90 is 3 x 3 tiles.
- rt_net_execute_frames_filtered: the frame path with one rt_disparity_speckle in front of the resampling, bit-equal to the op-level
  calls made by hand around rt_net_execute.
CPU tier: the same sources on the SIMT emulator, which runs workgroups one after another; GPU tier (-m gpu): the MI355X, plus one
full-size case, the only place where more workgroups run than the chip has compute units."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from oracle import stereo_oracle as O
from redtail_amd import capi, model_files, synth
from test_camera_frames import PAD, images, netlib, pack, rt, sample_bgr  # noqa: F401  (rt: the emu / gpu fixture)
from test_frames_any_size import call_ex, engine_by_hand, outputs, read
from test_lr_consistency import Bufs, make_net
from test_points import SENTINEL, bufs_3d, camera, compare_3d, read_points
from test_rectify import raw_pair, rectify_by_hand, rig

f32, u32 = np.float32, np.uint32
PIXELS, U16 = capi.RT_DISP_PIXELS_F32, capi.RT_DISP_KITTI_U16
CV, DOWN = capi.RT_RESIZE_CV_AREA, capi.RT_RESIZE_AREA_DOWN
M_F32, MM_U16 = capi.RT_DEPTH_M_F32, capi.RT_DEPTH_MM_U16
NAN, INF = float("nan"), float("inf")
TILE = 32
ALL = ("depth", "points", "compact")


# ---- the definition restated ----------------------------------------------------------------------------------------------------------------
def restate(px, mask, max_size, max_diff):
    """what rt_disparity_speckle must write, bit for bit: out, mask, valid_count.  px (N,1,H,W) float32, mask (N,1,H,W) uint8 or None"""
    px = np.asarray(px, f32)
    n, _, h, w = px.shape
    out, keep_all = np.zeros_like(px), np.zeros((n, 1, h, w), bool)
    idx = np.arange(h * w).reshape(h, w)
    for i in range(n):
        d = px[i, 0]
        live = ~np.isnan(d) if mask is None else ~np.isnan(d) & (np.asarray(mask)[i, 0] != 0)
        with np.errstate(invalid="ignore", over="ignore"):
            hz = live[:, :-1] & live[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= f32(max_diff))
            vt = live[:-1] & live[1:] & (np.abs(d[:-1] - d[1:]) <= f32(max_diff))
        a = np.concatenate([idx[:, :-1][hz], idx[:-1][vt]])
        b = np.concatenate([idx[:, 1:][hz], idx[1:][vt]])
        _, lab = connected_components(coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(h * w, h * w)), directed=False)
        sizes = np.bincount(lab[live.reshape(-1)], minlength=lab.max() + 1)
        keep = live & (sizes[lab].reshape(h, w) > max_size)
        keep_all[i, 0] = keep
        out[i, 0] = np.where(keep, d, f32(0))
    return dict(out=out, mask=keep_all * np.uint8(255), valid_count=keep_all.sum(axis=(1, 2, 3)).astype(np.uint64))


def workspace(k, d, n, h, w):
    """the op's workspace, filled with a pattern: nothing may depend on what it held"""
    return d.full((k.speckle_workspace_bytes(n, h, w),), np.uint8, 0xCD)


def run(k, d, px, mask, max_size, max_diff, in_place=False, want=("mask", "valid_count"), stream=None, sync=None):
    n, _, h, w = px.shape
    src, m = d.put(px), None if mask is None else d.put(mask)
    out = src if in_place else d.nan(n, 1, h, w)
    om = (m if in_place and m is not None else d.full((n, 1, h, w), np.uint8, 7)) if "mask" in want else None
    cnt = d.full((n,), np.uint64, 12345) if "valid_count" in want else None
    k.disparity_speckle(src, n, h, w, max_size, max_diff, out, mask=m, out_mask=om, valid_count=cnt, workspace=workspace(k, d, n, h, w),
                        stream=stream)
    if sync:
        sync()
    got = dict(out=d.get(out, f32))
    if om is not None:
        got["mask"] = d.get(om, np.uint8)
    if cnt is not None:
        got["valid_count"] = d.get(cnt, np.uint64)
    return got


def assert_bits(got, ref, what=""):
    for key, v in got.items():
        r = ref[key]
        assert v.dtype == r.dtype and v.shape == r.shape, (what, key, v.dtype, v.shape, r.dtype, r.shape)
        a, b = (v.view(u32), r.view(u32)) if v.dtype == f32 else (v, r)
        assert np.array_equal(a, b), (what, key, int((a != b).sum()))


def check(k, d, px, mask, max_size, max_diff, what, removed=None, kept=None):
    """the op against the restatement; removed / kept: the number of live pixels that must go / stay (None: at least one of each)"""
    ref = restate(px, mask, max_size, max_diff)
    live = ~np.isnan(px) if mask is None else ~np.isnan(px) & (mask != 0)
    n_kept = int(ref["valid_count"].sum())
    n_removed = int(live.sum()) - n_kept
    assert (n_kept > 0 if kept is None else n_kept == kept), (what, "kept", n_kept)
    assert (n_removed > 0 if removed is None else n_removed == removed), (what, "removed", n_removed)
    assert_bits(run(k, d, px, mask, max_size, max_diff), ref, what)
    return ref


# ---- 1. adversarial topologies, 3 x 3 tiles ---------------------------------------------------------------------------------------------------
H3, W3 = 70, 90


def serpentine(h, w):
    """value 5 along a snake: every even row, joined to the next even row at alternating ends; value 100 on the rest of the odd rows"""
    d = np.full((h, w), f32(100))
    d[0::2] = 5
    for j, y in enumerate(range(1, h - 1, 2)):
        d[y, w - 1 if j % 2 == 0 else 0] = 5
    return d[None, None]


def test_serpentine_through_every_tile(rt):
    """one component that crosses every tile border many times (the longest label chains); the 89-pixel rests of the odd rows go"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    px = serpentine(H3, W3)
    snake = int((px == 5).sum())
    check(k, d, px, None, W3, 1.0, "snake stays", removed=(H3 // 2 - 1) * (W3 - 1) + W3, kept=snake)          # (the last row, odd, is whole)
    check(k, d, px, None, snake - 1, 1.0, "snake is one component of exactly this size", removed=H3 * W3 - snake, kept=snake)
    check(k, d, px, None, snake, 1.0, "and goes at its own size", removed=H3 * W3, kept=0)
    check(k, d, px, None, 50, 95.0, "a max_diff that joins everything", removed=0, kept=H3 * W3)


def test_interleaved_combs(rt):
    """two combs whose teeth alternate column by column and differ by more than max_diff: two components, never one"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    h, w = H3, W3 - 1                                        # odd width: the combs differ in size
    px = np.zeros((1, 1, h, w), f32)
    px[0, 0, 0], px[0, 0, -1] = 10, 20
    px[0, 0, 1:-1, 0::2], px[0, 0, 1:-1, 1::2] = 10, 20
    a, b = int((px == 10).sum()), int((px == 20).sum())
    assert a > b
    check(k, d, px, None, b, 1.0, "the smaller comb goes", removed=b, kept=a)
    check(k, d, px, None, b - 1, 1.0, "both stay", removed=0, kept=a + b)
    check(k, d, px, None, a, 1.0, "both go", removed=a + b, kept=0)


def test_checkerboard_constant_and_ramp(rt):
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    yy, xx = np.meshgrid(np.arange(H3), np.arange(W3), indexing="ij")
    board = np.where((yy + xx) % 2 == 0, f32(1), f32(5))[None, None]
    check(k, d, board, None, 1, 1.0, "checkerboard: singletons", removed=H3 * W3, kept=0)
    check(k, d, board, None, 0, 1.0, "checkerboard, max_size 0", removed=0, kept=H3 * W3)
    const = np.full((1, 1, H3, W3), f32(3.5))
    check(k, d, const, None, H3 * W3 - 1, 0.0, "constant: one component, kept whole", removed=0, kept=H3 * W3)
    check(k, d, const, None, H3 * W3, 0.0, "constant at its own size", removed=H3 * W3, kept=0)
    ramp = (f32(0.5) * xx.astype(f32) + f32(0.25) * yy.astype(f32))[None, None]          # steps 0.5 / 0.25, end to end 62: > 50 x max_diff
    assert ramp.max() - ramp.min() > 50 * 0.5
    check(k, d, ramp, None, H3 * W3 - 1, 0.5, "ramp: neighbour to neighbour, not against a seed", removed=0, kept=H3 * W3)
    check(k, d, ramp, None, H3 - 1, 0.25, "ramp, columns only", removed=0, kept=H3 * W3)
    check(k, d, ramp, None, H3, 0.25, "ramp, columns only, at their size", removed=H3 * W3, kept=0)


def test_size_boundary_astride_tile_corners(rt):
    """rectangles of exactly max_size and max_size + 1 pixels over the corners (32, 32) and (64, 64): the first goes, the second stays"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    px = np.full((1, 1, H3, W3), NAN, f32)
    px[0, 0, 30:34, 29:34] = 7                               # 4 x 5 = 20 over (32, 32)
    px[0, 0, 62:65, 61:68] = 7                               # 3 x 7 = 21 over (64, 64)
    ref = check(k, d, px, None, 20, 0.0, "20 goes, 21 stays", removed=20, kept=21)
    assert ref["mask"][0, 0, 62:65, 61:68].all() and not ref["mask"][0, 0, 30:34, 29:34].any()
    check(k, d, px, None, 19, 0.0, "both stay", removed=0, kept=41)
    check(k, d, px, None, 21, 0.0, "both go", removed=41, kept=0)


def test_where_components_join_and_where_they_must_not(rt):
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    # a U whose arms live in tile (0, 0) and whose bottom lies in tile (1, 0); a second one without a bottom: two arms
    px = np.full((1, 1, H3, W3), NAN, f32)
    px[0, 0, 10:41, 5], px[0, 0, 10:41, 20], px[0, 0, 40, 5:21] = 2, 2, 2
    px[0, 0, 10:41, 25], px[0, 0, 10:41, 30] = 2, 2
    u = 31 + 31 + 14
    check(k, d, px, None, u - 1, 0.0, "the U is one component through the tile below", removed=62, kept=u)
    check(k, d, px, None, 30, 0.0, "arms of 31", removed=0, kept=u + 62)
    check(k, d, px, None, 31, 0.0, "arms of 31 go", removed=62, kept=u)
    # two 3 x 3 blobs in tiles (0, 0) and (0, 1) that touch at the one pixel pair (12, 31) - (12, 32)
    px = np.full((1, 1, H3, W3), NAN, f32)
    px[0, 0, 10:13, 29:32], px[0, 0, 12:15, 32:35] = 4, 4
    check(k, d, px, None, 17, 0.0, "joined: 18", removed=0, kept=18)
    check(k, d, px, None, 18, 0.0, "joined: 18 goes", removed=18, kept=0)
    px[0, 0, 12:15, 32:35] = 6
    check(k, d, px, None, 9, 1.0, "values 2 apart: two blobs of 9", removed=18, kept=0)
    # ... and down a column: (31, 40) - (32, 40)
    px = np.full((1, 1, H3, W3), NAN, f32)
    px[0, 0, 29:32, 40:43], px[0, 0, 32:35, 38:41] = 4, 4
    check(k, d, px, None, 17, 0.0, "joined across a horizontal border", removed=0, kept=18)
    # the end of a row does not touch the start of the next one
    px = np.full((1, 1, 37, 70), NAN, f32)
    px[0, 0, 5, 69], px[0, 0, 6, 0], px[0, 0, 20:22, 10:12] = 1, 1, 1
    check(k, d, px, None, 1, 0.0, "(y, W-1) and (y+1, 0) are two singletons", removed=2, kept=4)
    # the last row of image n does not touch the first row of image n + 1
    px = np.full((3, 1, 5, 7), NAN, f32)
    px[0, 0, 4], px[1, 0, 0], px[1, 0, 4], px[2, 0, 0], px[2, 0, 1] = 1, 1, 1, 1, 1
    check(k, d, px, None, 7, 0.0, "rows of 7 in neighbouring images", removed=21, kept=14)
    # a mask cuts a blob in two
    px = np.full((1, 1, 20, 40), f32(9))
    mask = np.full((1, 1, 20, 40), 255, np.uint8)
    mask[0, 0, :, 17] = 0
    check(k, d, px, mask, 340, 0.0, "17 columns go, 22 stay", removed=340, kept=440)
    check(k, d, px, None, 440, 0.0, "without the mask it is whole", removed=0, kept=800)


def test_special_values(rt):
    """a NaN is dead, an infinity is a live singleton (inf - inf is a NaN), -0.0 and 0.0 are adjacent at max_diff 0, max_size 0 removes nothing"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    rng = np.random.default_rng(5)
    px = np.full((2, 1, 37, 70), f32(1))
    where = rng.uniform(size=px.shape)
    px[where < 0.05], px[(where >= 0.05) & (where < 0.1)], px[(where >= 0.1) & (where < 0.15)] = NAN, INF, -INF
    px[0, 0, 3, 3:6] = INF                                   # neighbouring infinities of one sign stay singletons
    n_inf, n_nan = int(np.isinf(px).sum()), int(np.isnan(px).sum())
    ref = check(k, d, px, None, 1, 3e38, "infinities go alone")
    assert not ref["mask"][np.isinf(px)].any() and not ref["mask"][np.isnan(px)].any()
    ref = check(k, d, px, None, 0, 1.0, "max_size 0: mask = live, value or 0", removed=0, kept=px.size - n_nan)
    assert (ref["out"][np.isinf(px)] == px[np.isinf(px)]).all() and n_inf > 0
    zeros = np.where(rng.uniform(size=(1, 1, 33, 129)) < 0.5, f32(0.0), f32(-0.0))
    ref = check(k, d, zeros, None, 33 * 129 - 1, 0.0, "signed zeros are one component", removed=0, kept=33 * 129)
    assert np.array_equal(ref["out"].view(u32), zeros.view(u32))                            # the bits are copied: -0.0 stays -0.0
    levels = rng.integers(0, 3, (1, 1, 33, 129)).astype(f32)
    check(k, d, levels, None, 3, 0.0, "equality only")


# ---- 2. fuzz ----------------------------------------------------------------------------------------------------------------------------------
def piecewise(rng, n, h, w):
    """random piecewise-constant images on a grid of quarter pixels, with ~10 % masked, a few NaN and a few infinities"""
    bs = int(rng.integers(1, 7))
    coarse = rng.integers(0, 6, (n, 1, -(-h // bs), -(-w // bs))).astype(f32) * f32(0.5)
    px = np.kron(coarse, np.ones((bs, bs), f32))[:, :, :h, :w] + rng.integers(0, 2, (n, 1, h, w)).astype(f32) * f32(0.25)
    r = rng.uniform(size=px.shape)
    px[r < 0.01], px[(r >= 0.01) & (r < 0.02)] = NAN, INF
    mask = np.where(rng.uniform(size=px.shape) < 0.1, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(px, f32), mask


SHAPES = [(1, 37, 70), (2, 33, 129), (3, 1, 1), (1, 1, 97), (2, 97, 1), (3, 2, 2), (1, 70, 90), (2, 64, 64), (1, 65, 33)]


@pytest.mark.parametrize("seed", range(5))
def test_fuzz(rt, seed):
    """thresholds on exactly representable differences (0, 0.25, 0.5, 0.75 of a quarter-pixel grid); with and without the mask"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    rng = np.random.default_rng(100 + seed)
    for i, (n, h, w) in enumerate(SHAPES):
        px, mask = piecewise(rng, n, h, w)
        max_diff = (0.0, 0.25, 0.5, 0.75)[(i + seed) % 4]
        max_size = int(rng.integers(0, 12))
        m = mask if (i + seed) % 3 else None
        ref = restate(px, m, max_size, max_diff)
        assert_bits(run(k, d, px, m, max_size, max_diff), ref, (seed, n, h, w, max_diff, max_size))
        assert ref["valid_count"].sum() == (ref["mask"] != 0).sum()


# ---- 3. forms -----------------------------------------------------------------------------------------------------------------------------------
def test_forms(rt):
    """in place against out of place, every subset of the optional outputs, on a stream and on the NULL stream, two runs"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    px, mask = piecewise(np.random.default_rng(42), 2, 37, 70)
    ref = restate(px, mask, 6, 0.25)
    assert 0 < ref["valid_count"].sum() < (mask != 0).sum()
    assert np.array_equal(ref["valid_count"], (ref["mask"] != 0).sum(axis=(1, 2, 3)))
    first = run(k, d, px, mask, 6, 0.25)
    assert_bits(first, ref, "out of place")
    assert_bits(run(k, d, px, mask, 6, 0.25), first, "second run")
    assert_bits(run(k, d, px, mask, 6, 0.25, in_place=True), ref, "in place")
    assert_bits(run(k, d, px, None, 6, 0.25, in_place=True), restate(px, None, 6, 0.25), "in place, no input mask")
    for want in ((), ("mask",), ("valid_count",)):
        assert_bits(run(k, d, px, mask, 6, 0.25, want=want), ref, want)
        assert_bits(run(k, d, px, mask, 6, 0.25, want=want, in_place=True), ref, ("in place", want))
    if rt == "gpu":
        s = torch.cuda.Stream()
        stream, sync = s.cuda_stream, s.synchronize
        torch.cuda.synchronize()
    else:
        handle = ctypes.c_void_p()
        k.check(k.lib.rt_stream_create(ctypes.byref(handle)), "rt_stream_create")
        stream = handle.value
        sync = lambda: k.check(k.lib.rt_stream_sync(stream), "rt_stream_sync")      # noqa: E731
    assert_bits(run(k, d, px, mask, 6, 0.25, stream=stream, sync=sync), ref, "on a stream")
    assert_bits(run(k, d, px, mask, 0, 0.25, stream=stream, sync=sync), restate(px, mask, 0, 0.25), "on a stream, max_size 0")
    if rt != "gpu":
        k.lib.rt_stream_destroy(stream)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_op_refusals(rt):
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    n, h, w = 2, 9, 11
    px = d.put(np.ones((n, 1, h, w), f32))
    out, om, cnt = d.nan(n, 1, h, w), d.full((n, 1, h, w), np.uint8, 7), d.full((n,), np.uint64, 12345)
    ws = workspace(k, d, n, h, w)
    need = k.speckle_workspace_bytes(n, h, w)
    assert need > 0 and k.speckle_workspace_bytes(1, 1, 1) > 0 and k.speckle_workspace_bytes(32767, 1, 1) > 0
    for bad in ((0, h, w), (n, 0, w), (n, h, 0), (-1, h, w), (32768, h, w), (1, 1 << 16, 1 << 15), (1, 46341, 46341)):
        assert k.speckle_workspace_bytes(*bad) == 0, bad
    good = dict(disp=px, n=n, h=h, w=w, max_size=3, max_diff=1.0, out=out, workspace=ws, workspace_bytes=need)
    cases = [dict(disp=None), dict(out=None), dict(n=0), dict(h=0), dict(w=-1), dict(n=32768), dict(h=1 << 16, w=1 << 15), dict(max_size=-1),
             dict(max_diff=-1.0), dict(max_diff=NAN), dict(max_diff=INF), dict(workspace=None, workspace_bytes=0), dict(workspace=None),
             dict(workspace_bytes=need - 1)]
    for kw in cases:
        a = dict(good, **kw)
        with pytest.raises(capi.RtError):
            k.disparity_speckle(a["disp"], a["n"], a["h"], a["w"], a["max_size"], a["max_diff"], a["out"], out_mask=om, valid_count=cnt,
                                workspace=a["workspace"], workspace_bytes=a["workspace_bytes"])
        assert np.isnan(d.get(out)).all() and (d.get(om) == 7).all() and (d.get(cnt, np.uint64) == 12345).all(), kw
        assert (d.get(ws) == 0xCD).all(), kw
    k.disparity_speckle(px, n, h, w, 3, 1.0, out, out_mask=om, valid_count=cnt, workspace=ws)          # and the valid call next to them works
    assert (d.get(out) == 1).all() and (d.get(om) == 255).all() and (d.get(cnt, np.uint64) == h * w).all()


# ---- 5. rt_net_execute_frames_filtered on synthetic weights ------------------------------------------------------------------------------------------
# The synthetic networks' disparity is rough (neighbours differ by about a pixel), so speckle_size 6 / speckle_range 1 cuts it into pieces
# of which some are small: on every engine output of the cases below between a tenth and three quarters of the live pixels stay.  Each
# case asserts on the sequence by hand that pixels go and pixels stay.
FILTER = {"resnet18_2D": (6, 1.0), "nvtiny": (6, 1.0)}


def filtered_by_hand(lib, d, raw, n, h, w, scale, sh, sw, fl, step, enc, cam, max_diff, speckle, zmin, zmax, depth_kind, disp_kind):
    """the op-level calls behind rt_net_execute: rt_lr_consistency or rt_disparity_scale (or nothing), rt_disparity_speckle, then
    rt_disparity_to_points with every output and rt_disparity_to_frame.  Returns (points outputs, frame outputs, removed, kept)."""
    k = lib.kernels
    px, mask = d.nan(n, 1, h, w), d.full((n, 1, h, w), np.uint8, 7)
    ws = workspace(k, d, n, h, w)
    if max_diff >= 0:
        k.lr_consistency(raw, n, h, w, float(scale), max_diff, px, PIXELS, mask, None, None)
        before = int((d.get(mask) != 0).sum())
        k.disparity_speckle(px, n, h, w, speckle[0], speckle[1], px, mask=mask, out_mask=mask, workspace=ws)
    else:
        before = n * h * w
        if scale != 1:
            k.disparity_scale(raw, px, n * h * w, float(scale))
            k.disparity_speckle(px, n, h, w, speckle[0], speckle[1], px, out_mask=mask, workspace=ws)
        else:
            k.disparity_speckle(raw, n, h, w, speckle[0], speckle[1], px, out_mask=mask, workspace=ws)
    kept = int((d.get(mask) != 0).sum())
    b = bufs_3d(d, n, sh, sw, True, ALL, True, depth_kind, disp_kind)
    pws = d.full((k.points_workspace_bytes(n, sh, sw),), np.uint8, 0)
    k.disparity_to_points(px, n, h, w, sh, sw, cam, zmin, zmax, mask=mask, color=fl, color_step=step, encoding=enc, disp_out=b["disp"],
                          disp_kind=disp_kind, out_mask=b["mask"], valid_count=b["valid_count"], depth=b["depth"], depth_kind=depth_kind,
                          points=b["points"], points_compact=b["compact"], count=b["count"], workspace=pws)
    f = outputs(d, n, sh, sw, disp_kind)
    k.disparity_to_frame(px, n, h, w, f["out"], sh, sw, kind=disp_kind, mask=mask, out_mask=f["mask"], valid_count=f["valid_count"])
    return read_points(d, b, disp_kind, depth_kind), read(d, f, disp_kind), before - kept, kept


def call_filtered(net, fl, fr, enc, cam, b, n, resize, max_diff, speckle, zmin=0.0, zmax=INF, depth_kind=M_F32, disp_kind=PIXELS, **kw):
    net.execute_frames_filtered(fl, fr, enc, speckle_size=None if speckle is None else speckle[0],
                                speckle_range=1.0 if speckle is None else speckle[1], camera=cam, disp=b["disp"], kind=disp_kind, resize=resize,
                                max_diff_px=max_diff, mask=b["mask"], valid_count=b["valid_count"], min_depth=zmin, max_depth=zmax,
                                depth=b["depth"], depth_kind=depth_kind, points=b["points"], points_compact=b["compact"], count=b["count"],
                                batch=n, **kw)


@pytest.mark.parametrize("model", ["resnet18_2D", "nvtiny"])
def test_execute_frames_filtered_equals_the_pipeline_by_hand(rt, model):
    """With and without a check; with `out` (depth, organised and compact cloud), without it, and with `rect` (raw frames in): each
    bit-equal to the op-level calls by hand on the same engine, whose own mask shows that the filter removed pixels and kept pixels.
    ResNet-18 2D at batch 2 without a check and at batch 1 with one; NVTiny at batch 1, where no scale step runs and the filter works out
    of place.  (An engine pass on the emulator takes seconds: all cases run on the rectified frames, so that one pass by hand serves the
    three calls.)"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    net, h, w, scale = make_net(lib, model)
    enc = capi.RT_ENC_BGRA8
    speckle = FILTER[model]
    modes = [(CV, -1.0, 30, 36, M_F32, PIXELS), (DOWN, 1.5, 51, 83, MM_U16, U16)]
    for i, (resize, max_diff, sh, sw, depth_kind, disp_kind) in enumerate(modes):
        n = 2 if model == "resnet18_2D" and i == 0 else 1
        cl, cr = rig(k, sh, sw, fx=40.0)
        raw_l, raw_r = raw_pair(n, sh, sw, enc, PAD, seed=90 + i)
        fl, fr = d.put(raw_l), d.put(raw_r)
        rl, rr = rectify_by_hand(k, d, fl, fr, sh, sw, enc, cl, cr, n)
        step = rl.shape[2]
        cam = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)
        zmin, zmax = ((0.0, INF), (0.05, 1.0))[i % 2]
        raw = engine_by_hand(lib, d, net, rl, rr, sh, sw, step, enc, h, w, n, max_diff >= 0)
        ref3, ref2, removed, kept = filtered_by_hand(lib, d, raw, n, h, w, scale, sh, sw, rl, step, enc, cam, max_diff, speckle, zmin, zmax,
                                                     depth_kind, disp_kind)
        print(model, "check" if max_diff >= 0 else "no check", "removed", removed, "kept", kept)
        assert removed > 0 and kept > 0, (model, max_diff, removed, kept)
        # with `out`: every output at once
        b = bufs_3d(d, n, sh, sw, True, ALL, True, depth_kind, disp_kind)
        call_filtered(net, rl, rr, enc, cam, b, n, resize, max_diff, speckle, zmin, zmax, depth_kind, disp_kind, src_w=sw)
        compare_3d(read_points(d, b, disp_kind, depth_kind), ref3, n, sh * sw, (model, i, "out"))
        # without `out`: rt_disparity_to_frame behind the filter; mask and count are legal without a check
        f = outputs(d, n, sh, sw, disp_kind)
        net.execute_frames_filtered(rl, rr, enc, speckle_size=speckle[0], speckle_range=speckle[1], disp=f["out"], kind=disp_kind, resize=resize,
                                    max_diff_px=max_diff, mask=f["mask"], valid_count=f["valid_count"], batch=n, src_w=sw, no_depth_call=True)
        got = read(d, f, disp_kind)
        for key in ref2:
            assert np.array_equal(got[key], ref2[key]), (model, i, "no out", key)
        assert 0 < got["valid_count"].sum() < n * sh * sw
        # with `rect`: raw frames in, the cloud alone
        b = bufs_3d(d, n, sh, sw, False, ("compact",), False, depth_kind, disp_kind)
        call_filtered(net, fl, fr, enc, cam, b, n, resize, max_diff, speckle, zmin, zmax, depth_kind, disp_kind, src_w=sw, rect_left=cl, rect_right=cr)
        compare_3d(read_points(d, b, disp_kind, depth_kind), ref3, n, sh * sw, (model, i, "rect"))
    net.destroy()


def test_no_filter_is_the_wrapped_call_and_refusals_write_nothing(rt):
    """speckle == NULL: rt_net_execute_frames_raw / _3d / _ex on the same arguments.  RT_GEOM_NET with a filter: RT_E_UNSUPPORTED.  A wrong
    struct_bytes, a negative max_size, a bad max_diff_px, and a mask with neither a check nor a filter: an error, nothing written."""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    net, h, w, scale = make_net(lib, "resnet18_2D")
    n, enc, sh, sw = 1, capi.RT_ENC_BGRA8, 30, 36
    cl, cr = rig(k, sh, sw, fx=40.0)
    raw_l, raw_r = raw_pair(n, sh, sw, enc, PAD, seed=95)
    fl, fr = d.put(raw_l), d.put(raw_r)
    cam = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)
    # raw
    old, new = bufs_3d(d, n, sh, sw, True, ALL, True), bufs_3d(d, n, sh, sw, True, ALL, True)
    net.execute_frames_raw(fl, fr, enc, cl, cr, cam, disp=old["disp"], max_diff_px=1.5, mask=old["mask"], valid_count=old["valid_count"],
                           depth=old["depth"], points=old["points"], points_compact=old["compact"], count=old["count"], batch=n, src_w=sw)
    call_filtered(net, fl, fr, enc, cam, new, n, CV, 1.5, None, src_w=sw, rect_left=cl, rect_right=cr)
    ref = read_points(d, old, PIXELS, M_F32)
    assert 0 < ref["count"].sum()
    compare_3d(read_points(d, new, PIXELS, M_F32), ref, n, sh * sw, "raw")
    # 3d
    old, new = bufs_3d(d, n, sh, sw, True, ALL, False), bufs_3d(d, n, sh, sw, True, ALL, False)
    net.execute_frames_3d(fl, fr, enc, cam, disp=old["disp"], depth=old["depth"], points=old["points"], points_compact=old["compact"],
                          count=old["count"], batch=n, src_w=sw)
    call_filtered(net, fl, fr, enc, cam, new, n, CV, -1.0, None, src_w=sw)
    compare_3d(read_points(d, new, PIXELS, M_F32), read_points(d, old, PIXELS, M_F32), n, sh * sw, "3d")
    # ex
    old = read(d, call_ex(d, net, fl, fr, enc, n, sh, sw, PIXELS, capi.RT_GEOM_FRAME, CV, 1.5, src_w=sw), PIXELS)
    new = outputs(d, n, sh, sw, PIXELS)
    net.execute_frames_filtered(fl, fr, enc, disp=new["out"], max_diff_px=1.5, mask=new["mask"], valid_count=new["valid_count"], batch=n, src_w=sw,
                                no_depth_call=True)
    new = read(d, new, PIXELS)
    for key in old:
        assert np.array_equal(new[key], old[key]), ("ex", key)
    # refusals
    b = bufs_3d(d, n, sh, sw, True, ALL, True)

    def untouched():
        g = read_points(d, b, PIXELS, M_F32)
        return (np.isnan(g["disp"]).all() and (g["mask"] == 7).all() and (g["valid_count"] == 12345).all() and
                (g["depth"] == f32(1e30).view(u32)).all() and (g["points"].view(np.uint8) == SENTINEL).all() and
                (g["compact"].view(np.uint8) == SENTINEL).all() and (g["count"] == 12345).all())

    with pytest.raises(capi.RtError) as e:
        call_filtered(net, fl, fr, enc, cam, b, n, CV, 1.5, (5, 1.0), src_w=sw, geometry=capi.RT_GEOM_NET)
    assert "RT_GEOM_NET" in str(e.value) and "(%d)" % -2 in str(e.value) and untouched(), str(e.value)
    with pytest.raises(capi.RtError) as e:                 # ... also without `out`, where RT_GEOM_NET alone would be legal
        net.execute_frames_filtered(fl, fr, enc, speckle_size=5, disp=b["disp"], geometry=capi.RT_GEOM_NET, batch=n, src_w=sw, no_depth_call=True)
    assert "(%d)" % -2 in str(e.value) and untouched(), str(e.value)
    bad = [dict(speckle_struct_bytes=ctypes.sizeof(capi.SpeckleCall) - 8), dict(speckle_struct_bytes=0), dict(speckle=(-1, 1.0)),
           dict(speckle=(5, NAN)), dict(speckle=(5, -0.5)), dict(speckle=(5, INF)), dict(struct_bytes=ctypes.sizeof(capi.FrameCall) - 8),
           dict(depth_struct_bytes=ctypes.sizeof(capi.DepthCall) - 8), dict(rect_left=cl, rect_right=cr, rect_struct_bytes=ctypes.sizeof(capi.RectifyCall) - 8)]
    for kw in bad:
        kw = dict(kw)
        speckle = kw.pop("speckle", (5, 1.0))
        with pytest.raises(capi.RtError):
            call_filtered(net, fl, fr, enc, cam, b, n, CV, 1.5, speckle, src_w=sw, **kw)
        assert untouched(), kw
    for kw in (dict(), dict(rect_left=cl, rect_right=cr)):  # a mask with neither a check nor a filter is still refused
        with pytest.raises(capi.RtError) as e:
            call_filtered(net, fl, fr, enc, cam, b, n, CV, -1.0, None, src_w=sw, **kw)
        assert "need a check" in str(e.value) and untouched(), str(e.value)
    call_filtered(net, fl, fr, enc, cam, b, n, CV, -1.0, (5, 1.0), src_w=sw)               # ... and legal with a filter
    assert not untouched()
    net.destroy()


def test_filtered_in_graph_mode_with_rotating_buffers(rt):
    """a camera ring: three sets of frame and output buffers in rotation on a stream with graph mode on, then on the NULL stream: every
    call equal to the direct result.  (The emulator has no graphs: there the engine launches directly, and the rotation still runs.)"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    enc = capi.RT_ENC_BGRA8
    if rt == "gpu":
        n, h, w, sh, sw, md = 2, 129, 257, 120, 300, 16
    else:
        n, h, w, sh, sw, md = 1, 25, 41, 30, 36, 8
    net = lib.create("resnet18_2D", w, h, max_batch=2 * n, weights=O.synth_weights_resnet18_2d(), max_disp=md)
    cam = camera(fx=300.0, fy=300.0, cx=sw / 2 + 0.2, cy=sh / 2 - 0.3, baseline=0.2)
    sets = [(d.put(pack(images(n, sh, sw, 40 + 2 * i), enc, PAD, i)), d.put(pack(images(n, sh, sw, 41 + 2 * i), enc, PAD, i + 7))) for i in range(3)]
    # speckle_size 1 / speckle_range 2: behind the check these engines leave scattered pixels (155 on the emulator's 41 x 25 net, of which
    # 95 stay; 900 on the GPU's 257 x 129 net, of which 26 stay)
    speckle = (1, 2.0)

    def go(i, b, stream=None):
        call_filtered(net, sets[i][0], sets[i][1], enc, cam, b, n, CV, 1.0, speckle, 0.5, 60.0, src_w=sw, stream=stream)

    direct = []
    for i in range(3):
        b = bufs_3d(d, n, sh, sw, True, ALL, True)
        go(i, b)
        direct.append(read_points(d, b, PIXELS, M_F32))
    step = sets[0][0].shape[2]
    raw = engine_by_hand(lib, d, net, sets[0][0], sets[0][1], sh, sw, step, enc, h, w, n, True)
    ref3, _, removed, kept = filtered_by_hand(lib, d, raw, n, h, w, w, sh, sw, sets[0][0], step, enc, cam, 1.0, speckle, 0.5, 60.0, M_F32, PIXELS)
    assert removed > 0 and kept > 0, (removed, kept)
    compare_3d(direct[0], ref3, n, sh * sw, "direct")
    if rt == "gpu":
        s = torch.cuda.Stream()
        stream, sync = s.cuda_stream, s.synchronize
    else:
        handle = ctypes.c_void_p()
        k.check(k.lib.rt_stream_create(ctypes.byref(handle)), "rt_stream_create")
        stream = handle.value
        sync = lambda: k.check(k.lib.rt_stream_sync(stream), "rt_stream_sync")      # noqa: E731
    net.set_graph(True)
    for call in range(9 if rt == "gpu" else 3):            # 1: direct, 2: capture + launch, then replays, whatever pointers rotate in
        i = call % 3
        b = bufs_3d(d, n, sh, sw, True, ALL, True)           # fresh sentinel-filled buffers: other pointers on every call
        if rt == "gpu":
            torch.cuda.synchronize()
        go(i, b, stream=stream)
        sync()
        compare_3d(read_points(d, b, PIXELS, M_F32), direct[i], n, sh * sw, call)
    for call in range(3 if rt == "gpu" else 1):            # and on the NULL stream, synchronously
        i = (call + 1) % 3
        b = bufs_3d(d, n, sh, sw, True, ALL, True)
        go(i, b)
        compare_3d(read_points(d, b, PIXELS, M_F32), direct[i], n, sh * sw, ("null stream", call))
    net.destroy()
    if rt != "gpu":
        k.lib.rt_stream_destroy(stream)


# ---- 6. GPU only: full size -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_size_op():
    """1257 x 369, batch 2: 480 tiles per image, more workgroups than the chip has compute units, labels that cross XCDs"""
    k, d = netlib("gpu").kernels, Bufs(True)
    px, mask = synth.synth_speckle_disparity(2, 369, 1257)
    ref = restate(px, mask, 200, 1.0)
    removed = int((mask != 0).sum()) - int(ref["valid_count"].sum())
    print("full size: %d live, %d removed, %d kept" % ((mask != 0).sum(), removed, ref["valid_count"].sum()))
    assert removed > 1000 and ref["valid_count"].min() > 369 * 1257 // 2
    first = run(k, d, px, mask, 200, 1.0)
    assert_bits(first, ref, "full size")
    assert_bits(run(k, d, px, mask, 200, 1.0, in_place=True), ref, "full size, in place")
    assert_bits(run(k, d, px, None, 200, 1.0), restate(px, None, 200, 1.0), "full size, no mask: the zeros of the holes are live")


@pytest.mark.gpu
def test_full_size_sample_pair():
    """the reference's 1242 x 375 pair through ResNet-18 2D 1257 x 369 with trained weights, a check at 1 px and the node's usual
    speckle_size 200 / speckle_range 1 (scaled to this geometry they are the same numbers): equal to the sequence by hand"""
    lib, d = netlib("gpu"), Bufs(True)
    w, h = 1257, 369
    try:
        weights_path = model_files.weight_file("resnet18_2D")
    except FileNotFoundError as e:
        pytest.skip(str(e))
    net = lib.create("resnet18_2D", w, h, max_batch=2, weights_path=weights_path)
    left, right = sample_bgr()
    sh, sw = left.shape[1:3]
    enc = capi.RT_ENC_BGR8
    fl, fr = d.put(pack(left, enc)), d.put(pack(right, enc))
    cam = camera(fx=721.5377, fy=721.5377, cx=609.5593, cy=172.854, baseline=0.54)
    b = bufs_3d(d, 1, sh, sw, True, ALL, True)
    call_filtered(net, fl, fr, enc, cam, b, 1, CV, 1.0, (200, 1.0), src_w=sw)
    raw = engine_by_hand(lib, d, net, fl, fr, sh, sw, 3 * sw, enc, h, w, 1, True)
    ref3, _, removed, kept = filtered_by_hand(lib, d, raw, 1, h, w, w, sh, sw, fl, 3 * sw, enc, cam, 1.0, (200, 1.0), 0.0, INF, M_F32, PIXELS)
    print("sample pair: the filter removed %d of %d checked pixels" % (removed, removed + kept))
    assert removed > 0 and kept > 0
    compare_3d(read_points(d, b, PIXELS, M_F32), ref3, 1, sh * sw, "sample pair")
    net.destroy()
