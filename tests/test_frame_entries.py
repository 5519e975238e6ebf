"""State shared between the seven camera-frame entries of one net.

Every other frame test holds one entry bit-equal to op-level calls made by hand.  What they leave open is what the entries share on a
net: the three engine bindings, the network-geometry pixels and mask, the grow-on-demand workspaces (rectified frames, compact cloud),
the speckle workspace.  Here one net runs all seven entries at batch 1 and 2 in a fixed interleaved order -- SEQUENCE below -- and every
output of every call must be bit-equal to the same call on a freshly created net that has run nothing else; then the same sequence
once more on a stream with graph mode on.

Each call writes into one sentinel-filled arena that holds every output the entries know, a guard in front of, between and behind
them; only the outputs the call asks for are passed.  After the call everything else in the arena must still be the sentinel.
Refused calls stand between the others: they write nothing and report what a fresh net reports.

Frames: 36 x 30 bgra8 with padded rows into the 41 x 25 net for the entries that take any size.  RT_RESIZE_AREA_DOWN (the only filter
of rt_net_execute_frames, _lr and _viz) refuses frames narrower than the network, so those entries get 83 x 51 frames, which are also
the larger size at which rt_net_execute_frames_raw makes the net's rectified frames and cloud workspace grow.
CPU tier: the same sources on the SIMT emulator, a part of the order (EMU below); GPU tier (-m gpu): the MI355X, all of it."""
import numpy as np
import pytest
import torch

from redtail_amd import capi
from test_camera_frames import PAD, netlib, rt  # noqa: F401  (rt: the emu / gpu fixture)
from test_lr_consistency import Bufs, make_net
from test_points import camera
from test_rectify import raw_pair, rig
from test_viz import MAX_DISP, make_stream

NET, PIXELS, U16 = capi.RT_DISP_NET, capi.RT_DISP_PIXELS_F32, capi.RT_DISP_KITTI_U16
CV, DOWN = capi.RT_RESIZE_CV_AREA, capi.RT_RESIZE_AREA_DOWN
G_NET, G_FRAME = capi.RT_GEOM_NET, capi.RT_GEOM_FRAME
ENC = capi.RT_ENC_BGRA8
FILL, GUARD = 0xA5, 64                                   # the sentinel byte; bytes between two outputs (keeps the clouds on 16 bytes)
SMALL, LARGE = (30, 36), (51, 83)                        # (rows, columns) of the two frame sizes
SPECKLE = (6, 1.0)
CLOUD = ("depth", "compact", "count")


class Arena:
    """one device buffer with a span for every output an entry can write; `want`: the ones this call passes"""

    def __init__(self, d, sizes, want):
        self.d, self.want, self.spans, off = d, want, {}, GUARD
        for name, nbytes in sizes.items():
            self.spans[name] = (off, nbytes)
            off += -(-nbytes // GUARD) * GUARD + GUARD
        self.buf = d.full((off,), np.uint8, FILL)

    def __getitem__(self, name):
        if name not in self.want:
            return None
        off, nbytes = self.spans[name]
        return self.buf[off:off + nbytes]

    def read(self, refused=False):
        """the requested outputs as bytes; guards and outputs not asked for (after a refusal: everything) must be untouched"""
        got = self.d.get(self.buf, np.uint8)
        asked = np.zeros(got.size, bool)
        out = {}
        for name in () if refused else self.want:
            off, nbytes = self.spans[name]
            asked[off:off + nbytes] = True
            out[name] = got[off:off + nbytes].copy()
            assert (out[name] != FILL).any(), name + " was not written"
        assert (got[~asked] == FILL).all(), "%d bytes written outside the requested outputs" % int((got[~asked] != FILL).sum())
        return out


class Step:
    def __init__(self, entry, size, n, want, geometry=G_FRAME, resize=CV, max_diff=-1.0, kind=PIXELS, rect=False, speckle=None, out=True,
                 refused=False):
        if entry in ("frames", "lr", "viz"):             # the entries with flat arguments: the network's geometry, down-scaling only
            geometry, resize = G_NET, DOWN
        self.entry, self.size, self.n, self.want, self.geometry, self.resize, self.max_diff, self.kind = entry, size, n, want, geometry, resize, max_diff, kind
        self.rect, self.speckle, self.out, self.refused = rect, speckle, out, refused

    def run(self, ctx, net, stream=None, sync=None):
        d, n, (sh, sw) = ctx.d, self.n, self.size
        oh, ow = (sh, sw) if self.geometry == G_FRAME else (ctx.h, ctx.w)
        plane, px, vstep = n * oh * ow, (2 if self.kind == U16 else 4), 6 * ctx.w + PAD
        a = Arena(d, dict(disp=plane * px, disp_right=plane * px, mask=plane, valid_count=8 * n, depth=4 * plane, points=16 * plane,
                          compact=16 * plane, count=8 * n, viz=n * 2 * ctx.h * vstep), self.want)
        fl, fr = ctx.frames[self.size]
        cl, cr = ctx.rigs[self.size] if self.rect else (None, None)
        common = dict(batch=n, stream=stream, src_w=sw)
        call = dict(kind=self.kind, geometry=self.geometry, resize=self.resize, max_diff_px=self.max_diff, mask=a["mask"], valid_count=a["valid_count"])
        cloud = dict(min_depth=0.05, max_depth=40.0, depth=a["depth"], points=a["points"], points_compact=a["compact"], count=a["count"],
                     no_depth_call=not self.out)
        if ctx.gpu:
            torch.cuda.synchronize()                     # the arena was filled on torch's stream
        try:
            if self.entry == "frames":
                net.execute_frames(fl, fr, ENC, a["disp"], kind=self.kind, **common)
            elif self.entry == "lr":
                net.execute_frames_lr(fl, fr, ENC, a["disp"], kind=self.kind, mask=a["mask"], disp_right=a["disp_right"],
                                      valid_count=a["valid_count"], max_diff_px=self.max_diff, **common)
            elif self.entry == "viz":
                net.execute_frames_viz(fl, fr, ENC, a["disp"], a["viz"], viz_step=vstep, max_disp=MAX_DISP, max_diff_px=self.max_diff,
                                       mask=a["mask"], valid_count=a["valid_count"], **common)
            elif self.entry == "ex":
                net.execute_frames_ex(fl, fr, ENC, a["disp"], **call, **common)
            elif self.entry == "3d":
                net.execute_frames_3d(fl, fr, ENC, ctx.cams[self.size], disp=a["disp"], **call, **cloud, **common)
            elif self.entry == "raw":
                net.execute_frames_raw(fl, fr, ENC, cl, cr, ctx.cams[self.size], disp=a["disp"], **call, **cloud, **common)
            else:
                net.execute_frames_filtered(fl, fr, ENC, speckle_size=self.speckle and self.speckle[0],
                                            speckle_range=self.speckle[1] if self.speckle else 1.0, rect_left=cl, rect_right=cr,
                                            camera=ctx.cams[self.size], disp=a["disp"], **call, **cloud, **common)
            error = None
        except capi.RtError as e:
            error = str(e)
        if sync:
            sync()
        assert (error is not None) == self.refused, (self.entry, error)
        got = a.read(self.refused)
        if error:
            got["error"] = error
        return got


# the fixed order; the comments name what a call shares with the ones before it
SEQUENCE = [
    Step("filtered", SMALL, 1, ("disp", "mask", "valid_count") + CLOUD, max_diff=1.5, rect=True, speckle=SPECKLE),    # 0: everything on
    Step("frames", LARGE, 2, ("disp",)),                                                                              # 1: bindings only
    Step("lr", LARGE, 1, ("disp", "mask", "disp_right", "valid_count"), max_diff=1.0, kind=U16),                      # 2
    Step("ex", LARGE, 2, ("disp",), geometry=G_NET, resize=DOWN),                                                     # 3 = 1
    Step("ex", LARGE, 1, ("disp", "mask", "valid_count"), geometry=G_NET, resize=DOWN, max_diff=1.0, kind=U16),       # 4 = 2
    Step("frames", SMALL, 2, ("disp",), refused=True),                                                                # 5: up-scaling
    Step("viz", LARGE, 1, ("disp", "viz")),                                                                           # 6
    Step("viz", LARGE, 2, ("disp", "mask", "valid_count", "viz"), max_diff=1.0),                                      # 7
    Step("raw", LARGE, 2, ("disp", "points") + CLOUD, rect=True),                                                     # 8: rect, points_ws grow
    Step("filtered", LARGE, 2, ("disp", "points") + CLOUD, rect=True),                                                # 9 = 8
    Step("filtered", SMALL, 1, ("disp",), geometry=G_NET, speckle=SPECKLE, refused=True),                             # 10: unsupported
    Step("3d", SMALL, 2, ("disp", "mask", "valid_count"), max_diff=1.5, kind=U16, out=False),                         # 11
    Step("ex", SMALL, 2, ("disp", "mask", "valid_count"), max_diff=1.5, kind=U16),                                    # 12 = 11
    Step("filtered", SMALL, 1, ("disp",) + CLOUD),                                                                    # 13
    Step("3d", SMALL, 1, ("disp",) + CLOUD),                                                                          # 14 = 13
    Step("lr", LARGE, 1, ("disp", "mask"), max_diff=-1.0, refused=True),                                              # 15: needs a tolerance
    Step("filtered", SMALL, 2, ("disp", "mask", "valid_count") + CLOUD, max_diff=1.5, rect=True, speckle=SPECKLE),    # 16: 0 at batch 2
    Step("frames", LARGE, 1, ("disp",), kind=NET),                                                                    # 17
]
SAME = [(3, 1), (4, 2), (9, 8), (12, 11), (14, 13)]      # (call, the entry it stands for): equal in every output of the first
# The emulator takes about six seconds per image of an engine pass and has no graphs.  It runs this part of the order -- a call with
# everything on (check, filter, rectified frames, cloud), then the network-geometry entries at batch 2 and 1 that must not find its
# buffers in their way, the cloud without check or filter, and the three refusals -- and one call on a stream.  The GPU runs all of it.
EMU, STREAM_EMU = (0, 1, 5, 6, 10, 13, 15), (6,)


class Context:
    def __init__(self, lib, d, gpu, h, w):
        self.lib, self.d, self.gpu, self.h, self.w = lib, d, gpu, h, w
        self.frames, self.rigs, self.cams = {}, {}, {}
        for i, (sh, sw) in enumerate((SMALL, LARGE)):
            left, right = raw_pair(2, sh, sw, ENC, PAD, seed=60 + i)
            self.frames[sh, sw] = d.put(left), d.put(right)
            self.rigs[sh, sw] = rig(lib.kernels, sh, sw, fx=40.0)
            self.cams[sh, sw] = camera(fx=30.0, fy=31.0, cx=sw / 2 - 0.3, cy=sh / 2 + 0.2, baseline=0.1, doffs=0.5)


def assert_same(got, ref, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for key, v in got.items():
        if key == "error":
            assert v == ref[key], (what, v, ref[key])
        else:
            assert v.shape == ref[key].shape and np.array_equal(v, ref[key]), (what, key, int((v != ref[key]).sum()))


def test_entries_share_one_net(rt):
    lib, d = netlib(rt), Bufs(rt == "gpu")
    shared, h, w, _ = make_net(lib, "resnet18_2D", max_batch=4)
    ctx = Context(lib, d, rt == "gpu", h, w)
    order = [(i, step) for i, step in enumerate(SEQUENCE) if rt == "gpu" or i in EMU]
    alone = {}
    for i, step in order:                                # every call on a net of its own
        net = make_net(lib, "resnet18_2D", max_batch=4)[0]
        alone[i] = step.run(ctx, net)
        net.destroy()
    for i, j in SAME:
        if i in alone and j in alone:
            for key in alone[i]:
                assert np.array_equal(alone[i][key], alone[j][key]), (i, j, key)
    for i, step in order:
        if "valid_count" in step.want:                   # the check, and the filter behind it, keep some pixels and drop some
            oh, ow = step.size if step.geometry == G_FRAME else (h, w)
            assert 0 < alone[i]["valid_count"].view(np.uint64).sum() < step.n * oh * ow, i
        if "count" in step.want:
            assert alone[i]["count"].view(np.uint64).sum() > 0, i
    for i, step in order:                                # all calls on one net, NULL stream
        assert_same(step.run(ctx, shared), alone[i], ("shared", i, step.entry))
    stream, sync, destroy, keep = make_stream(lib, rt == "gpu")
    shared.set_graph(True)                               # ... and once more on a stream with graph mode on
    for i, step in order:
        if rt == "gpu" or i in STREAM_EMU:
            assert_same(step.run(ctx, shared, stream, sync), alone[i], ("graph", i, step.entry))
    destroy()
    shared.destroy()
