"""The cloud on a voxel grid: pcl::VoxelGrid behind stereo_image_proc/point_cloud2, on the device.

- rt_points_voxel_grid: one record per occupied cell -- centroid from 16-bit offsets, mean colour -- in ascending cell index.  `restate`
  below says include/rt_stereo.h's definition again with numpy float32 operations, np.unique on the cell, np.add.at on integers and
  float64 for the centroid's offset -- another algorithm than the kernels' bitmap, ranks and atomics -- and every case is bit-exact
  against it, sentinel bytes behind the last record included.  The only tolerance is the accuracy case's, which is derived there.
  The kernels scan the bitmap in blocks of SCAN_WORDS words of 32 cells and hand a lane RUN consecutive records: the grids and the
  point counts sit astride those.
- rt_net_execute_frames_voxels: the frame path with one rt_points_voxel_grid behind the cloud, bit-equal to
  rt_net_execute_frames_camera followed by the op by hand.
CPU tier: the same sources on the SIMT emulator; GPU tier (-m gpu): the MI355X, plus one full-size case, the only place where the atomics
cross XCDs and more workgroups run than the chip has compute units."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import stereo_oracle as O
from redtail_amd import capi
from test_camera_frames import PAD, images, netlib, pack, rt  # noqa: F401  (rt: the emu / gpu fixture)
from test_decode import new_stream, wire_rows
from test_lr_consistency import Bufs, make_net
from test_points import SENTINEL, bufs_3d, camera, compare_3d, read_points
from test_rectify import raw_pair, rig

f32, f64, u32, u64, i64 = np.float32, np.float64, np.uint32, np.uint64, np.int64
NAN, INF = float("nan"), float("inf")
PIXELS, M_F32 = capi.RT_DISP_PIXELS_F32, capi.RT_DEPTH_M_F32
CV = capi.RT_RESIZE_CV_AREA
SCAN_WORDS, RUN = 1024, 4                                  # voxel.hip.h: kVoxelScan, kVoxelRun
WS_FILL = 0xCD


def make_grid(origin, leaf, dims):
    return capi.VoxelGrid.make(origin, leaf, dims)


# ---- the definition restated ----------------------------------------------------------------------------------------------------------------
def restate(pts, grid, counts=None, min_points=1, out_capacity=None):
    """what rt_points_voxel_grid must leave in sentinel-filled outputs, bit for bit.  pts (n, capacity, 4) uint32 records {x, y, z bits, rgb};
    counts (n,) or None.  Returns voxels (n, out_capacity, 4) uint32, count (n,) uint64, cell and n (n, out_capacity) uint32, and per image
    the full lists (cells, N, records) under "all"."""
    pts = np.asarray(pts, u32)
    n, cap = pts.shape[:2]
    oc = cap if out_capacity is None else out_capacity
    origin, leaf = np.array(list(grid.origin), f32), np.array(list(grid.leaf), f32)
    dims = np.array(list(grid.dims), i64)
    sent = u32(SENTINEL * 0x01010101)
    out = dict(voxels=np.full((n, oc, 4), sent, u32), count=np.zeros(n, u64), cell=np.full((n, oc), sent, u32), n=np.full((n, oc), sent, u32), all=[])
    for i in range(n):
        recs = pts[i, :cap if counts is None else min(int(counts[i]), cap)]
        xyz, rgb = np.ascontiguousarray(recs[:, :3]).view(f32), recs[:, 3]
        with np.errstate(invalid="ignore", over="ignore"):
            t = (xyz - origin[None, :]) / leaf[None, :]                                   # float32, each operation rounded on its own
            inside = np.all((t >= f32(0)) & (t < dims.astype(f32)[None, :]), axis=1)
        t, rgb = t[inside], rgb[inside]
        fl = np.floor(t)
        idx = fl.astype(i64)
        cell = (idx[:, 2] * dims[1] + idx[:, 1]) * dims[0] + idx[:, 0]
        q = ((t - fl) * f32(65536)).astype(u32).astype(i64)
        assert q.size == 0 or (q.min() >= 0 and q.max() <= 65535)
        cells, inv = np.unique(cell, return_inverse=True)
        N, S, C = np.zeros(cells.size, i64), np.zeros((cells.size, 3), i64), np.zeros((cells.size, 3), i64)
        np.add.at(N, inv, 1)
        np.add.at(S, inv, q)
        np.add.at(C, inv, np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], axis=1).astype(i64))
        keep = N >= min_points
        cells, N, S, C = cells[keep], N[keep], S[keep], C[keep]
        g = (S.astype(f64) / N[:, None].astype(f64) + 0.5) / 65536.0
        ci = np.stack([cells % dims[0], cells // dims[0] % dims[1], cells // (dims[0] * dims[1])], axis=1)
        corner = origin[None, :] + ci.astype(f32) * leaf[None, :]
        c = corner + g.astype(f32) * leaf[None, :]
        assert c.dtype == f32 and corner.dtype == f32
        col = (C + (N // 2)[:, None]) // N[:, None]
        rec = np.concatenate([c.view(u32), ((col[:, 0] << 16) | (col[:, 1] << 8) | col[:, 2]).astype(u32)[:, None]], axis=1)
        m = min(oc, cells.size)
        out["voxels"][i, :m], out["cell"][i, :m], out["n"][i, :m] = rec[:m], cells[:m].astype(u32), N[:m].astype(u32)
        out["count"][i] = cells.size
        out["all"].append((cells, N, rec))
    return out


def records(xyz, rgb=None):
    """(n, capacity, 3) float32 positions (+ (n, capacity) uint32 colours) -> (n, capacity, 4) uint32 records"""
    xyz = np.asarray(xyz, f32)
    rgb = np.zeros(xyz.shape[:2], u32) if rgb is None else np.asarray(rgb, u32)
    return np.concatenate([np.ascontiguousarray(xyz).view(u32), rgb[..., None]], axis=2)


def workspace(k, d, n, cap, grid):
    """the op's workspace, filled with a pattern: nothing may depend on what it held"""
    need = k.voxel_workspace_bytes(n, cap, grid)
    assert need > 0
    return d.full((need,), np.uint8, WS_FILL)


def run(k, d, pts, grid, counts=None, min_points=1, out_capacity=None, want=("cell", "n"), stream=None, sync=None, ws=None):
    pts = np.asarray(pts, u32)
    n, cap = pts.shape[:2]
    oc = cap if out_capacity is None else out_capacity
    src = d.put(np.ascontiguousarray(pts).view(np.uint8))
    cnt = None if counts is None else d.put(np.asarray(counts, u64).view(i64))
    vox, oc_buf = d.full((n, oc, 16), np.uint8, SENTINEL), d.full((n,), u64, 12345)
    cell = d.full((n, oc, 4), np.uint8, SENTINEL) if "cell" in want else None
    num = d.full((n, oc, 4), np.uint8, SENTINEL) if "n" in want else None
    k.points_voxel_grid(src, n, cap, grid, vox, oc, oc_buf, count=cnt, min_points=min_points, out_cell=cell, out_n=num,
                        workspace=workspace(k, d, n, cap, grid) if ws is None else ws, stream=stream)
    if sync:
        sync()
    got = dict(voxels=np.ascontiguousarray(d.get(vox)).view(u32), count=d.get(oc_buf, u64))
    if cell is not None:
        got["cell"] = np.ascontiguousarray(d.get(cell)).view(u32).reshape(n, oc)
    if num is not None:
        got["n"] = np.ascontiguousarray(d.get(num)).view(u32).reshape(n, oc)
    assert np.array_equal(np.ascontiguousarray(d.get(src)).view(u32).reshape(pts.shape), pts)          # the input is read only
    return got


def assert_bits(got, ref, what=""):
    for key, v in got.items():
        r = ref[key]
        assert v.dtype == r.dtype and v.shape == r.shape, (what, key, v.dtype, v.shape, r.dtype, r.shape)
        assert np.array_equal(v, r), (what, key, int((v != r).sum()), np.argwhere(v != r)[:4].tolist())


def check(k, d, pts, grid, what, emitted=None, **kw):
    """the op against the restatement; emitted: the number of voxels per image that must come out (None: at least one)"""
    ref = restate(pts, grid, kw.get("counts"), kw.get("min_points", 1), kw.get("out_capacity"))
    if emitted is None:
        assert ref["count"].sum() > 0, what
    else:
        assert ref["count"].tolist() == list(emitted), (what, ref["count"].tolist())
    assert_bits(run(k, d, pts, grid, **kw), ref, what)
    return ref


def centres(cells, grid, jitter=None):
    """a point inside each of the given cells: the centre, or the corner + jitter (in leaves, [0, 1))"""
    dims, leaf, origin = list(grid.dims), np.array(list(grid.leaf), f64), np.array(list(grid.origin), f64)
    cells = np.asarray(cells, i64)
    idx = np.stack([cells % dims[0], cells // dims[0] % dims[1], cells // (dims[0] * dims[1])], axis=1).astype(f64)
    j = 0.5 if jitter is None else jitter
    return (origin + (idx + j) * leaf).astype(f32)


# ---- 1. word and block borders ----------------------------------------------------------------------------------------------------------------
BORDER_GRID = make_grid((0.0, 0.0, 0.0), 0.5, (37, 33, 31))                               # 37 851 cells: 1 183 words, two scan blocks


def test_word_and_block_borders(rt):
    """37 x 33 x 31 = 37 851 cells is no multiple of 32 and spans two scan blocks.  Occupied: bits 0 and 31 of a word, the first and last
    word of the first block, the first word of the second, the last word (27 cells wide), the last cell of the grid; then every cell."""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    g = BORDER_GRID
    cells_total = 37 * 33 * 31
    words = -(-cells_total // 32)
    assert cells_total % 32 != 0 and SCAN_WORDS < words < 2 * SCAN_WORDS
    last_word = words - 1
    cells = [0, 31, 32, 63, 64 + 5, 32 * (SCAN_WORDS - 1), 32 * (SCAN_WORDS - 1) + 31, 32 * SCAN_WORDS, 32 * SCAN_WORDS + 31, 32 * last_word,
             cells_total - 1, 32 * 500 + 17]
    rng = np.random.default_rng(1)
    rep = np.repeat(cells, 3)                              # three points a cell, shuffled, 36 + 1 records: no multiple of RUN
    rng.shuffle(rep)
    xyz = centres(rep, g, rng.uniform(0.05, 0.95, (rep.size, 3)))
    xyz = np.concatenate([xyz, [[NAN, 1.0, 1.0]]]).astype(f32)
    rgb = rng.integers(0, 1 << 24, xyz.shape[0]).astype(u32)
    ref = check(k, d, records(xyz[None], rgb[None]), g, "borders", emitted=[len(cells)])
    assert ref["all"][0][0].tolist() == sorted(cells) and (ref["all"][0][1] == 3).all()
    # every cell of the grid once, in a random order: all words full, every rank used
    order = rng.permutation(cells_total)
    ref = check(k, d, records(centres(order, g)[None]), g, "every cell", emitted=[cells_total])
    assert np.array_equal(ref["cell"][0], np.arange(cells_total, dtype=u32))
    # a grid of one cell, and of one word exactly
    one = make_grid((-1.0, -1.0, -1.0), 2.0, (1, 1, 1))
    xyz = rng.uniform(-1.5, 1.5, (1, 41, 3)).astype(f32)
    ref = check(k, d, records(xyz), one, "one cell", emitted=[1])
    assert 0 < ref["n"][0, 0] < 41
    check(k, d, records(centres(rng.permutation(32), make_grid((0, 0, 0), 1.0, (4, 4, 2)))[None]), make_grid((0, 0, 0), 1.0, (4, 4, 2)), "one word",
          emitted=[32])


# ---- 2. collisions ----------------------------------------------------------------------------------------------------------------------------
def test_collisions(rt):
    """5 001 points (no multiple of the lane run or of 64) in one voxel: N and the sums exact; 5 001 points in 5 001 voxels"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    rng = np.random.default_rng(2)
    m = 5001
    assert m % RUN != 0 and m % 64 != 0
    g = make_grid((-1000.25, 3.5, 0.125), (0.25, 0.5, 0.125), (40, 20, 30))
    cell = (7 * 20 + 11) * 40 + 13
    xyz = centres(np.full(m, cell), g, rng.uniform(0.01, 0.99, (m, 3)))             # (0.01 leaves: far more than an ulp at 1000)
    rgb = rng.integers(0, 1 << 24, m).astype(u32)
    ref = check(k, d, records(xyz[None], rgb[None]), g, "one voxel", emitted=[1])
    assert ref["n"][0, 0] == m and ref["cell"][0, 0] == cell
    bright = np.full(m, 0xFFFFFF, u32)                                               # the largest colour sums
    ref = check(k, d, records(centres(np.full(m, cell), g)[None], bright[None]), g, "one voxel, white", emitted=[1])
    assert ref["n"][0, 0] == m and ref["voxels"][0, 0, 3] == 0xFFFFFF
    cells = rng.permutation(40 * 20 * 30)[:m]
    ref = check(k, d, records(centres(cells, g)[None], rgb[None]), g, "all apart", emitted=[m])
    assert (ref["n"][0, :m] == 1).all()
    # runs of equal cells of every length inside and across the lanes' four records
    runs = np.repeat(np.arange(300), rng.integers(1, 7, 300))
    ref = check(k, d, records(centres(runs * 3, g, rng.uniform(0.1, 0.9, (runs.size, 3)))[None]), g, "runs", emitted=[300])


# ---- 3. membership ----------------------------------------------------------------------------------------------------------------------------
def test_membership(rt):
    """faces, the origin, the far face, one ulp inside and outside it, -0.f offsets, NaN / inf / mixed records, a far-away origin with
    anisotropic leaves"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    nx = lambda v, to: np.nextafter(f32(v), f32(to))      # noqa: E731
    g = make_grid((0.0, 0.0, 0.0), 0.5, (4, 3, 2))
    far = (2.0, 1.5, 1.0)
    pts = [(0, 0, 0), (-0.0, -0.0, -0.0), (0.5, 0.5, 0.5), (1.0, 0.25, 0.25), (0.25, 1.0, 0.75),
           (far[0], 0.1, 0.1), (0.1, far[1], 0.1), (0.1, 0.1, far[2]), far,                       # on the far faces: out
           (nx(far[0], 0), 0.1, 0.1), (0.1, nx(far[1], 0), 0.1), (0.1, 0.1, nx(far[2], 0)),       # just inside
           (nx(far[0], 9), 0.1, 0.1), (nx(0, -1), 0.1, 0.1), (0.1, nx(0, -1), 0.1),               # just outside
           (NAN, 0.1, 0.1), (0.1, NAN, 0.1), (0.1, 0.1, NAN), (NAN, NAN, NAN), (INF, 0.1, 0.1), (0.1, -INF, 0.1), (INF, NAN, -INF),
           (1.9, 1.4, 0.9), (-3.0, 0.1, 0.1), (0.1, 7.0, 0.1)]
    xyz = np.array(pts, f32)[None]
    rgb = np.arange(1, xyz.shape[1] + 1, dtype=u32)[None] * u32(0x010203)
    ref = check(k, d, records(xyz, rgb), g, "faces")
    t_in = [0, 1, 2, 3, 4, 9, 10, 11, 22]
    assert int(ref["all"][0][1].sum()) == len(t_in)
    assert ref["all"][0][0][0] == 0 and ref["all"][0][1][0] == 2                                  # 0.f and -0.f share cell 0
    # a far-away origin, anisotropic leaves: the cell corner is rounded before the offset is added
    g = make_grid((-1000.25, 3.5, 0.125), (0.3, 0.07, 1.1), (50, 60, 7))
    rng = np.random.default_rng(3)
    lo, hi = np.array([-1000.25, 3.5, 0.125]), np.array([-1000.25 + 15.0, 3.5 + 4.2, 0.125 + 7.7])
    xyz = rng.uniform(lo - 0.5, hi + 0.5, (1, 3001, 3)).astype(f32)
    ref = check(k, d, records(xyz, rng.integers(0, 1 << 24, (1, 3001)).astype(u32)), g, "far origin")
    assert 1500 < ref["all"][0][1].sum() < 3001 and ref["count"][0] > 1000


# ---- 4. order-freedom -------------------------------------------------------------------------------------------------------------------------
def surface(n, h, w, seed, hole=0.2):
    """an organised cloud: a smooth surface seen through a pinhole, NaN where there is a hole; and its compact form with counts"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=f64), np.arange(w, dtype=f64), indexing="ij")
    org, comp, counts = np.zeros((n, h * w, 4), u32), np.full((n, h * w, 4), u32(SENTINEL * 0x01010101)), np.zeros(n, u64)
    fx = 0.6 * w
    for i in range(n):
        z = 6.0 + 2.0 * np.sin(xx / w * 5.0 + i) + 1.5 * np.cos(yy / h * 3.0) + (xx > 0.6 * w) * 1.5
        xyz = np.stack([(xx - w / 2) / fx * z, (yy - h / 2) / fx * z, z], axis=2).astype(f32).reshape(-1, 3)
        rgb = rng.integers(0, 1 << 24, h * w).astype(u32)
        holes = rng.uniform(size=h * w) < hole
        xyz[holes] = NAN
        org[i] = records(xyz[None], rgb[None])[0]
        valid = org[i][~holes]
        comp[i, :valid.shape[0]], counts[i] = valid, valid.shape[0]
    return org, comp, counts


SURFACE_GRID = make_grid((-6.0, -4.0, 2.0), 0.5, (24, 16, 20))            # a few pixels of `surface` at 59 x 37 per cell


def test_order_freedom(rt):
    """a random permutation of an image's records changes no bit; the organised cloud with count == NULL and the compact cloud with its
    count give the same bytes; two runs agree"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    org, comp, counts = surface(2, 37, 59, 4)
    g = SURFACE_GRID
    ref = check(k, d, org, g, "organised")
    assert 100 < ref["count"].min() and ref["count"].max() < counts.min() and ref["n"][0, :int(ref["count"][0])].max() > 3
    first = run(k, d, org, g)
    assert_bits(run(k, d, org, g), first, "second run")
    assert_bits(run(k, d, comp, g, counts=counts), first, "compact with its count")
    rng = np.random.default_rng(5)
    shuffled = np.stack([org[i][rng.permutation(org.shape[1])] for i in range(2)])
    assert not np.array_equal(shuffled, org)
    assert_bits(run(k, d, shuffled, g), first, "permuted")
    assert_bits(run(k, d, org[:, ::-1], g), first, "reversed")


# ---- 5. forms ---------------------------------------------------------------------------------------------------------------------------------
def test_min_points(rt):
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    org, _, _ = surface(2, 37, 59, 6)
    g = SURFACE_GRID
    numbers = []
    for mp in (1, 2, 5):
        ref = check(k, d, org, g, ("min_points", mp), min_points=mp)
        numbers.append(int(ref["count"].sum()))
        assert all((ref["n"][i, :int(ref["count"][i])] >= mp).all() for i in range(2))
    assert numbers[0] > numbers[1] > numbers[2] > 0, numbers
    check(k, d, org, g, "min_points above every N", emitted=[0, 0], min_points=10000)
    # more slots than one scan block, min_points 2: ranks of the second scan cross a block border
    rng = np.random.default_rng(7)
    big = make_grid((0.0, 0.0, 0.0), 1.0, (64, 64, 2))
    cells = np.concatenate([np.arange(3000), rng.permutation(3000)[:1700]])
    rng.shuffle(cells)
    ref = check(k, d, records(centres(cells, big)[None]), big, "two blocks of slots", emitted=[1700], min_points=2)
    assert 3000 > SCAN_WORDS * 2 and ref["cell"][0, 1699] > SCAN_WORDS


def test_out_capacity_and_optional_outputs(rt):
    """out_capacity below the emitted number: out_count is the full number, exactly the first records are written, the sentinel behind
    them is intact; out_cell_u32 and out_n_u32 each alone, both and neither"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    org, _, _ = surface(2, 37, 59, 8)
    g = SURFACE_GRID
    full = restate(org, g)
    small = int(full["count"].min()) // 2 + 1
    for mp in (1, 2):
        ref = check(k, d, org, g, ("truncated", mp), out_capacity=small, min_points=mp)
        assert (ref["count"] > small).all() and ref["voxels"].shape == (2, small, 4)
    ref = check(k, d, org, g, "roomy", out_capacity=org.shape[1] + 7)
    assert (ref["voxels"][0, int(ref["count"][0]):].view(np.uint8) == SENTINEL).all()
    check(k, d, org, g, "one record", out_capacity=1)
    for want in ((), ("cell",), ("n",), ("cell", "n")):
        got = run(k, d, org, g, want=want)
        assert set(got) == {"voxels", "count"} | set(want)
        assert_bits(got, full, want)


def test_batch_of_three_with_counts(rt):
    """counts (k, 0, capacity): a partly filled image, an empty one and a full one, and nothing leaks from one image into the next;
    a count above the capacity reads the capacity"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    rng = np.random.default_rng(9)
    cap = 1003
    g = make_grid((-2.0, -2.0, -2.0), 0.5, (8, 8, 8))
    xyz = rng.uniform(-2.2, 2.2, (3, cap, 3)).astype(f32)
    pts = records(xyz, rng.integers(0, 1 << 24, (3, cap)).astype(u32))
    counts = np.array([317, 0, cap], u64)
    ref = check(k, d, pts, g, "counts", counts=counts)
    assert ref["count"][1] == 0 and 0 < ref["count"][0] < ref["count"][2]
    assert (ref["voxels"][1].view(np.uint8) == SENTINEL).all()
    assert int(ref["all"][0][1].sum()) <= 317
    over = np.array([cap + 5, 1 << 40, 1], u64)
    assert_bits(run(k, d, pts, g, counts=over), restate(pts, g, np.array([cap, cap, 1])), "count above capacity")
    check(k, d, pts, g, "counts, min_points 3", counts=counts, min_points=3)


def test_workspace_and_stream(rt):
    """the workspace holds 0xCD before the first call and the first call's leftovers before the second, whose input is another; on a
    stream"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    a, _, _ = surface(2, 37, 59, 10)
    b, _, _ = surface(2, 37, 59, 11, hole=0.6)
    g = SURFACE_GRID
    ws = workspace(k, d, 2, a.shape[1], g)
    ref_a, ref_b = restate(a, g, min_points=2), restate(b, g)
    assert not np.array_equal(ref_a["count"], ref_b["count"])
    assert_bits(run(k, d, a, g, min_points=2, ws=ws), ref_a, "first use")
    assert not (d.get(ws) == WS_FILL).all()
    assert_bits(run(k, d, b, g, ws=ws), ref_b, "second use, another input")
    assert_bits(run(k, d, a, g, min_points=2, ws=ws), ref_a, "third use")
    stream, sync, done = new_stream(rt, k)
    if rt == "gpu":
        torch.cuda.synchronize()
    assert_bits(run(k, d, a, g, min_points=2, ws=ws, stream=stream, sync=sync), ref_a, "on a stream")
    assert_bits(run(k, d, b, g, stream=stream, sync=sync), ref_b, "on a stream, min_points 1")
    done()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_op_refusals(rt):
    """every refusal of rt_points_voxel_grid: an error, sentinel-filled outputs and the workspace untouched; rt_voxel_workspace_bytes is 0
    for what the op refuses"""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    n, cap, oc = 2, 24, 24
    good_grid = make_grid((0.0, 0.0, 0.0), 0.5, (4, 4, 4))
    rng = np.random.default_rng(12)
    pts = records(rng.uniform(0, 2, (n, cap, 3)).astype(f32))
    src = d.put(pts.view(np.uint8))
    cnt = d.put(np.array([5, 7], u64).view(i64))
    vox, ocnt = d.full((n, oc, 16), np.uint8, SENTINEL), d.full((n,), u64, 12345)
    cell, num = d.full((n, oc, 4), np.uint8, SENTINEL), d.full((n, oc, 4), np.uint8, SENTINEL)
    need = k.voxel_workspace_bytes(n, cap, good_grid)
    ws = d.full((need + 16,), np.uint8, WS_FILL)
    assert need > 0 and k.voxel_workspace_bytes(1, 1, make_grid((0, 0, 0), 1.0, (1, 1, 1))) > 0
    assert k.voxel_workspace_bytes(32767, 1 << 23, make_grid((0, 0, 0), 1.0, (4096, 4096, 8))) > 0
    # a 2^27-cell grid costs one bit and one prefix word per 32 cells, not gigabytes: 32 MiB + what the 1000 slots and the block sums take
    assert k.voxel_workspace_bytes(1, 1000, make_grid((0, 0, 0), 0.05, (512, 512, 512))) < (32 << 20) + (1 << 17)
    bad_grids = [((0, 0, 0), 0.5, (0, 4, 4)), ((0, 0, 0), 0.5, (4, 4097, 4)), ((0, 0, 0), 0.5, (4, 4, -1)), ((0, 0, 0), 0.5, (4096, 4096, 9)),
                 ((0, 0, 0), 0.5, (1024, 1024, 129)), ((0, 0, 0), (0.5, 0.0, 0.5), (4, 4, 4)), ((0, 0, 0), (0.5, 0.5, -0.5), (4, 4, 4)),
                 ((0, 0, 0), (NAN, 0.5, 0.5), (4, 4, 4)), ((0, 0, 0), (0.5, INF, 0.5), (4, 4, 4)), ((NAN, 0, 0), 0.5, (4, 4, 4)),
                 ((0, -INF, 0), 0.5, (4, 4, 4)), ((0, 0, INF), 0.5, (4, 4, 4))]
    for bg in bad_grids:
        assert k.voxel_workspace_bytes(n, cap, make_grid(*bg)) == 0, bg
    for bad in ((0, cap), (-1, cap), (32768, cap), (n, 0), (n, -3), (n, (1 << 23) + 1)):
        assert k.voxel_workspace_bytes(bad[0], bad[1], good_grid) == 0, bad
    assert k.voxel_workspace_bytes(n, cap, None) == 0
    good = dict(points=src, n=n, cap=cap, grid=good_grid, vox=vox, oc=oc, ocnt=ocnt, count=cnt, mp=1, cell=cell, num=num, ws=ws, wsb=need)
    p = capi._ptr
    cases = [dict(points=None), dict(grid=None), dict(vox=None), dict(ocnt=None), dict(n=0), dict(n=-1), dict(n=32768), dict(cap=0),
             dict(cap=(1 << 23) + 1), dict(oc=0), dict(oc=-1), dict(oc=(1 << 23) + 1), dict(mp=0), dict(mp=-2), dict(points=p(src) + 4),
             dict(points=p(src) + 8), dict(vox=p(vox) + 4), dict(ws=None, wsb=0), dict(ws=None), dict(wsb=need - 1), dict(wsb=0),
             dict(vox=src), dict(vox=p(src) + 16 * cap), dict(ocnt=cnt), dict(cell=src), dict(num=p(src) + 64), dict(ws=src, wsb=1 << 30),
             dict(cell=vox), dict(num=cell)]
    cases += [dict(grid=make_grid(*bg)) for bg in bad_grids]
    for kw in cases:
        a = dict(good, **kw)
        with pytest.raises(capi.RtError):
            k.points_voxel_grid(a["points"], a["n"], a["cap"], a["grid"], a["vox"], a["oc"], a["ocnt"], count=a["count"], min_points=a["mp"],
                                out_cell=a["cell"], out_n=a["num"], workspace=a["ws"], workspace_bytes=a["wsb"])
        assert (d.get(vox) == SENTINEL).all() and (d.get(ocnt, u64) == 12345).all() and (d.get(cell) == SENTINEL).all(), kw
        assert (d.get(num) == SENTINEL).all() and (d.get(ws) == WS_FILL).all(), kw
        assert np.array_equal(np.ascontiguousarray(d.get(src)).view(u32).reshape(pts.shape), pts), kw
    k.points_voxel_grid(src, n, cap, good_grid, vox, oc, ocnt, count=cnt, out_cell=cell, out_n=num, workspace=ws, workspace_bytes=need)
    got = dict(voxels=np.ascontiguousarray(d.get(vox)).view(u32), count=d.get(ocnt, u64), cell=np.ascontiguousarray(d.get(cell)).view(u32).reshape(n, oc),
               n=np.ascontiguousarray(d.get(num)).view(u32).reshape(n, oc))
    assert_bits(got, restate(pts, good_grid, [5, 7]), "the valid call next to them")
    assert (d.get(ws)[need:] == WS_FILL).all()


# ---- 7. accuracy ------------------------------------------------------------------------------------------------------------------------------
def test_accuracy_against_the_float64_mean(rt):
    """|c_a - mean64_a| <= leaf_a * 2^-17 + 4 * 2^-24 * max(|origin_a|, |origin_a + dims_a * leaf_a|), the mean of the cell's points in
    float64.  From the definition: q_a truncates the offset inside the cell to 2^-16 leaves and g_a adds half a step back, so a point's
    offset is off by at most half a step, leaf_a * 2^-17, and so is their mean; the roundings of p_a - origin_a and of t_a (each half an
    ulp of a value below the grid's extent), of the cell corner (half an ulp of a coordinate inside the grid) and of the final sum (the
    same) are each at most 2^-24 times the largest coordinate magnitude of the grid: four of them.  The restatement alone must meet the
    bound on these inputs before the device is asked."""
    k, d = netlib(rt).kernels, Bufs(rt == "gpu")
    rng = np.random.default_rng(13)
    for origin, leaf, dims in (((-1000.25, 3.5, 0.125), (0.3, 0.07, 1.1), (50, 60, 7)), ((-4.0, -2.0, 0.5), (0.05, 0.05, 0.05), (160, 80, 100)),
                               ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (30, 30, 30))):
        g = make_grid(origin, leaf, dims)
        o, lf, dm = np.array(origin, f64), np.array(leaf, f64), np.array(dims, f64)
        m = 4001
        hot = o + rng.uniform(0.2, 0.8, 3) * dm * lf       # half of the points around one spot: voxels with many points
        xyz = np.where(rng.uniform(size=(m, 1)) < 0.5, rng.uniform(o, o + dm * lf, (m, 3)), hot + rng.normal(0, 2.0, (m, 3)) * lf).astype(f32)
        pts = records(xyz[None])
        ref = restate(pts, g)
        cells, N, rec = ref["all"][0]
        assert N.max() >= 5 and cells.size > 500
        # the float64 mean per voxel, with the restatement's own membership (float32 t)
        with np.errstate(invalid="ignore"):
            t = (xyz - np.array(origin, f32)) / np.array(leaf, f32)
        inside = np.all((t >= 0) & (t < np.array(dims, f32)), axis=1)
        idx = np.floor(t[inside]).astype(i64)
        cell = (idx[:, 2] * dims[1] + idx[:, 1]) * dims[0] + idx[:, 0]
        uniq, inv = np.unique(cell, return_inverse=True)
        assert np.array_equal(uniq, cells)
        mean = np.zeros((cells.size, 3), f64)
        np.add.at(mean, inv, xyz[inside].astype(f64))
        mean /= N[:, None]
        bound = lf * 2.0 ** -17 + 4 * 2.0 ** -24 * np.maximum(np.abs(o), np.abs(o + dm * lf))
        err = np.abs(rec[:, :3].view(f32).astype(f64) - mean)
        print("accuracy", origin, "max error / bound per axis", (err.max(axis=0) / bound).round(3))
        assert (err <= bound[None, :]).all(), ("the restatement", (err / bound).max())
        got = run(k, d, pts, g)
        err = np.abs(got["voxels"][0, :cells.size, :3].view(f32).astype(f64) - mean)
        assert (err <= bound[None, :]).all(), ("the device", (err / bound).max())
        assert_bits(got, ref, origin)


# ---- 8. rt_net_execute_frames_voxels ------------------------------------------------------------------------------------------------------------
ENTRY_GRID = make_grid((-1.0, -1.0, 0.0), 0.05, (40, 40, 40))             # the small nets' clouds lie within two metres
ALL = ("depth", "points", "compact")


def voxel_bufs(d, n, cap):
    return dict(voxels=d.full((n, cap, 16), np.uint8, SENTINEL), voxel_count=d.full((n,), u64, 12345), voxel_cell=d.full((n, cap, 4), np.uint8, SENTINEL),
                voxel_n=d.full((n, cap, 4), np.uint8, SENTINEL))


def read_voxels(d, v):
    n, cap = v["voxels"].shape[:2]
    return dict(voxels=np.ascontiguousarray(d.get(v["voxels"])).view(u32), count=d.get(v["voxel_count"], u64),
                cell=np.ascontiguousarray(d.get(v["voxel_cell"])).view(u32).reshape(n, cap), n=np.ascontiguousarray(d.get(v["voxel_n"])).view(u32).reshape(n, cap))


def voxels_untouched(d, v):
    return ((d.get(v["voxels"]) == SENTINEL).all() and (d.get(v["voxel_count"], u64) == 12345).all() and (d.get(v["voxel_cell"]) == SENTINEL).all() and
            (d.get(v["voxel_n"]) == SENTINEL).all())


def frame_kw(b, cam, n, max_diff, zmin, zmax, **kw):
    return dict(camera=cam, disp=b["disp"], resize=CV, max_diff_px=max_diff, mask=b["mask"], valid_count=b["valid_count"], min_depth=zmin,
                max_depth=zmax, depth=b["depth"], points=b["points"], points_compact=b["compact"], count=b["count"], batch=n, **kw)


def op_by_hand(k, d, cloud, n, records, grid, min_points, cap):
    v = voxel_bufs(d, n, cap)
    k.points_voxel_grid(cloud, n, records, grid, v["voxels"], cap, v["voxel_count"], min_points=min_points, out_cell=v["voxel_cell"],
                        out_n=v["voxel_n"], workspace=workspace(k, d, n, records, grid))
    return read_voxels(d, v)


def camera_then_op(lib, d, net, fl, fr, enc, cam, n, sh, sw, max_diff, zmin, zmax, grid, min_points, cap, wire=None, **kw):
    """the definition: rt_net_execute_frames_camera with every output, then rt_points_voxel_grid by hand on its organised cloud.  Returns
    the camera call's outputs, the voxels, and the organised cloud on the device"""
    check = max_diff >= 0 or kw.get("speckle_size") is not None
    b = bufs_3d(d, n, sh, sw, True, ALL, check)
    net.execute_frames_camera(fl, fr, wire, enc, **frame_kw(b, cam, n, max_diff, zmin, zmax, **kw))
    return read_points(d, b, PIXELS, M_F32), op_by_hand(lib.kernels, d, b["points"], n, sh * sw, grid, min_points, cap), b["points"]


def test_execute_frames_voxels_equals_camera_then_op(rt):
    """three calls, each against rt_net_execute_frames_camera followed by the op by hand: the caller's organised cloud with a check and a
    filter; the caller's compact cloud from raw frames (rectification); no cloud output at all -- no output pointer at all -- from Bayer
    frames (decode) at batch 2, min_points 2, a capacity below the emitted number"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    net, h, w, scale = make_net(lib, "resnet18_2D")
    enc, sh, sw = capi.RT_ENC_BGRA8, 30, 36
    cam = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)
    cl, cr = rig(k, sh, sw, fx=40.0)
    g = ENTRY_GRID
    # (a) the caller's organised cloud, a check and a filter
    n = 1
    raw_l, raw_r = raw_pair(n, sh, sw, enc, PAD, seed=70)
    fl, fr = d.put(raw_l), d.put(raw_r)
    ref3, refv, _ = camera_then_op(lib, d, net, fl, fr, enc, cam, n, sh, sw, 1.5, 0.0, INF, g, 1, sh * sw, src_w=sw, speckle_size=2, speckle_range=1.0)
    print("check + filter: %d points, %d voxels" % (ref3["count"].sum(), refv["count"].sum()))
    assert 0 < refv["count"].sum() < ref3["count"].sum()
    b, v = bufs_3d(d, n, sh, sw, True, ("depth", "points"), True), voxel_bufs(d, n, sh * sw)
    net.execute_frames_voxels(fl, fr, enc, grid=g, **v, **frame_kw(b, cam, n, 1.5, 0.0, INF, src_w=sw, speckle_size=2, speckle_range=1.0))
    compare_3d(read_points(d, b, PIXELS, M_F32), ref3, n, sh * sw, "organised")
    assert_bits(read_voxels(d, v), refv, "organised")
    # (b) the caller's compact cloud, raw frames in, a depth range
    ref3, refv, _ = camera_then_op(lib, d, net, fl, fr, enc, cam, n, sh, sw, -1.0, 0.05, 1.0, g, 1, sh * sw, src_w=sw, rect_left=cl, rect_right=cr)
    print("rectified: %d points, %d voxels" % (ref3["count"].sum(), refv["count"].sum()))
    assert 0 < refv["count"].sum() < ref3["count"].sum() <= n * sh * sw
    b, v = bufs_3d(d, n, sh, sw, False, ("compact",), False), voxel_bufs(d, n, sh * sw)
    net.execute_frames_voxels(fl, fr, enc, grid=g, **v, **frame_kw(b, cam, n, -1.0, 0.05, 1.0, src_w=sw, rect_left=cl, rect_right=cr))
    compare_3d(read_points(d, b, PIXELS, M_F32), ref3, n, sh * sw, "compact")
    assert_bits(read_voxels(d, v), refv, "compact")
    # (c) nothing but voxels, wire frames in, batch 2
    n, wire, enc3 = 2, capi.RT_WIRE_BAYER_GRBG8, capi.RT_ENC_RGB8
    wl, wr = (d.put(wire_rows(n, sh, sw, wire, s)) for s in (71, 72))
    full3, fullv, cloud = camera_then_op(lib, d, net, wl, wr, enc3, cam, n, sh, sw, -1.0, 0.0, INF, g, 2, sh * sw, wire=wire)
    print("bayer: %s points, %s voxels of two points or more" % (full3["count"].tolist(), fullv["count"].tolist()))
    cap = int(fullv["count"].min()) - 3
    assert cap > 0
    refv = op_by_hand(k, d, cloud, n, sh * sw, g, 2, cap)
    assert np.array_equal(refv["count"], fullv["count"]) and np.array_equal(refv["voxels"], fullv["voxels"][:, :cap])
    b, v = bufs_3d(d, n, sh, sw, False, (), False), voxel_bufs(d, n, cap)
    assert all(x is None for x in b.values())
    net.execute_frames_voxels(wl, wr, enc3, grid=g, min_points=2, wire_encoding=wire, **v, **frame_kw(b, cam, n, -1.0, 0.0, INF))
    assert_bits(read_voxels(d, v), refv, "voxels alone")
    net.destroy()


def test_no_voxel_call_is_the_wrapped_call_and_refusals_write_nothing(rt):
    """voxel == NULL: rt_net_execute_frames_camera on the same arguments, an error text included.  out == NULL, a wrong struct_bytes, a bad
    grid and whatever else only the voxel call can get wrong: an error, every sentinel-filled output untouched."""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    net, h, w, scale = make_net(lib, "resnet18_2D")
    n, enc, sh, sw = 1, capi.RT_ENC_BGRA8, 30, 36
    fl, fr = d.put(pack(images(n, sh, sw, 73), enc, PAD, 1)), d.put(pack(images(n, sh, sw, 74), enc, PAD, 2))
    cam = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)
    old, new = bufs_3d(d, n, sh, sw, True, ALL, False), bufs_3d(d, n, sh, sw, True, ALL, False)           # (no check: an engine pass on the emulator takes seconds)
    net.execute_frames_camera(fl, fr, None, enc, **frame_kw(old, cam, n, -1.0, 0.0, INF, src_w=sw))
    net.execute_frames_voxels(fl, fr, enc, **frame_kw(new, cam, n, -1.0, 0.0, INF, src_w=sw))
    ref = read_points(d, old, PIXELS, M_F32)
    assert ref["count"].sum() > 0
    compare_3d(read_points(d, new, PIXELS, M_F32), ref, n, sh * sw, "voxel == NULL")
    texts = []
    for call in (lambda **kw: net.execute_frames_camera(fl, fr, None, enc, **kw), lambda **kw: net.execute_frames_voxels(fl, fr, enc, **kw)):
        with pytest.raises(capi.RtError) as e:
            call(**frame_kw(new, cam, n, -1.0, 2.0, 1.0, src_w=sw))
        texts.append(str(e.value).replace("rt_net_execute_frames_camera", "*").replace("rt_net_execute_frames_voxels", "*"))
    assert texts[0] == texts[1] and "max_depth" in texts[0], texts
    # refusals
    b, v = bufs_3d(d, n, sh, sw, True, ALL, False), voxel_bufs(d, n, sh * sw)

    def untouched():
        g = read_points(d, b, PIXELS, M_F32)
        return (np.isnan(g["disp"]).all() and
                (g["depth"] == f32(1e30).view(u32)).all() and (g["points"].view(np.uint8) == SENTINEL).all() and
                (g["compact"].view(np.uint8) == SENTINEL).all() and (g["count"] == 12345).all() and voxels_untouched(d, v))

    p = capi._ptr
    bad = [dict(no_depth_call=True), dict(voxel_struct_bytes=ctypes.sizeof(capi.VoxelCall) - 8), dict(voxel_struct_bytes=0),
           dict(grid=make_grid((0, 0, 0), 0.25, (0, 32, 32))), dict(grid=make_grid((0, 0, 0), 0.25, (4096, 4096, 9))),
           dict(grid=make_grid((0, 0, 0), (0.25, NAN, 0.25), (32, 32, 32))), dict(grid=make_grid((0, INF, 0), 0.25, (32, 32, 32))),
           dict(min_points=0), dict(voxels=None), dict(voxel_count=None), dict(voxel_capacity=0), dict(voxel_capacity=(1 << 23) + 1),
           dict(voxels=p(v["voxels"]) + 4, voxel_capacity=8), dict(voxels=b["points"], voxel_capacity=8), dict(voxel_cell=b["points"]),
           dict(voxel_n=v["voxel_cell"]), dict(depth_struct_bytes=0), dict(struct_bytes=0), dict(geometry=capi.RT_GEOM_NET), dict(batch=0),
           dict(max_depth=-1.0)]
    for kw in bad:
        a = dict(grid=ENTRY_GRID, **v)
        a.update(frame_kw(b, cam, n, -1.0, 0.0, INF, src_w=sw))
        a.update(kw)
        with pytest.raises(capi.RtError) as e:
            net.execute_frames_voxels(fl, fr, enc, **a)
        assert "rt_net_execute_frames_voxels" in str(e.value), str(e.value)
        assert untouched(), kw
    net.execute_frames_voxels(fl, fr, enc, grid=ENTRY_GRID, **v, **frame_kw(b, cam, n, -1.0, 0.0, INF, src_w=sw))
    assert not untouched() and d.get(v["voxel_count"], u64)[0] > 0
    net.destroy()


def test_voxels_in_graph_mode_with_rotating_buffers(rt):
    """a camera ring: sets of frames and fresh output buffers in rotation on a stream with graph mode on, then on the NULL stream: every
    call equal to the direct result, which equals the camera call plus the op by hand.  (The emulator has no graphs: there the engine
    launches directly and the rotation still runs -- over two sets and without a check, since an engine pass takes seconds there.)"""
    lib, d = netlib(rt), Bufs(rt == "gpu")
    k = lib.kernels
    enc = capi.RT_ENC_BGRA8
    if rt == "gpu":
        n, h, w, sh, sw, md, ring, check = 2, 129, 257, 120, 300, 16, 3, 1.0
    else:
        n, h, w, sh, sw, md, ring, check = 1, 25, 41, 30, 36, 8, 2, -1.0
    net = lib.create("resnet18_2D", w, h, max_batch=2 * n, weights=O.synth_weights_resnet18_2d(), max_disp=md)
    cam = camera(fx=300.0, fy=300.0, cx=sw / 2 + 0.2, cy=sh / 2 - 0.3, baseline=0.2)
    g = make_grid((-8.0, -4.0, 0.0), (0.5, 0.25, 0.5), (32, 32, 130))
    sets = [(d.put(pack(images(n, sh, sw, 80 + 2 * i), enc, PAD, i)), d.put(pack(images(n, sh, sw, 81 + 2 * i), enc, PAD, i + 7))) for i in range(ring)]
    cap = sh * sw

    def go(i, v, stream=None):
        b = bufs_3d(d, n, sh, sw, False, (), False)
        net.execute_frames_voxels(sets[i][0], sets[i][1], enc, grid=g, min_points=1, **v, **frame_kw(b, cam, n, check, 0.5, 60.0, src_w=sw, stream=stream))

    direct = []
    for i in range(ring):
        v = voxel_bufs(d, n, cap)
        go(i, v)
        direct.append(read_voxels(d, v))
    _, refv, _ = camera_then_op(lib, d, net, sets[0][0], sets[0][1], enc, cam, n, sh, sw, check, 0.5, 60.0, g, 1, cap, src_w=sw)
    assert refv["count"].sum() > 0 and not np.array_equal(direct[0]["voxels"], direct[1]["voxels"])
    assert_bits(direct[0], refv, "direct")
    stream, sync, done = new_stream(rt, k)
    net.set_graph(True)
    for call in range(9 if rt == "gpu" else 2):
        i = call % ring
        v = voxel_bufs(d, n, cap)                           # fresh sentinel-filled buffers: other pointers on every call
        if rt == "gpu":
            torch.cuda.synchronize()
        go(i, v, stream=stream)
        sync()
        assert_bits(read_voxels(d, v), direct[i], call)
    for call in range(3 if rt == "gpu" else 1):
        i = (call + 1) % ring
        v = voxel_bufs(d, n, cap)
        go(i, v)
        assert_bits(read_voxels(d, v), direct[i], ("null stream", call))
    net.destroy()
    done()


# ---- 9. GPU only: full size ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_size_cloud():
    """a 1257 x 369 organised cloud (a smooth surface with a step, 20 % holes) on a 0.05 m grid of 9.6 million cells: 453 workgroups of
    records, atomics across XCDs; bit-exact against the restatement, twice, and with min_points 3"""
    k, d = netlib("gpu").kernels, Bufs(True)
    org, _, counts = surface(1, 369, 1257, 14)
    g = make_grid((-10.0, -3.0, 1.9), 0.05, (400, 120, 200))
    ref = restate(org, g)
    print("full size: %d points, %d voxels, largest N %d" % (counts[0], ref["count"][0], ref["all"][0][1].max()))
    assert ref["all"][0][1].sum() == counts[0] and 10000 < ref["count"][0] < counts[0]
    first = run(k, d, org, g)
    assert_bits(first, ref, "full size")
    assert_bits(run(k, d, org, g), first, "full size, second run")
    assert_bits(run(k, d, org, g, min_points=3), restate(org, g, min_points=3), "full size, min_points 3")
