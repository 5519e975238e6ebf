"""Op-level parity at the geometry bench.py times, for launches of C2 (ResNet-18 2D fp32, 1257x369, batch 1; one stream per context, so
every launch carries RT_HINT_THROUGHPUT -- engine.cpp: streams_ == 1).  Each case builds its plan through the C ABI with the setters the
engine applies to that layer, asserts from the RT_CONV_TRACE line which kernel, variant, grid and split ran, and compares the stored
output, decoded, with an fp64 evaluation of the same operation (oracle/stereo_oracle.py) at every output element.

Bounds come from the arithmetic.  The split-fp16 fp32 path (conv_split.hip.h, conv_rbs.hip.h, conv_rbd.hip.h, corr_mfma.hip.h) carries
each operand as hi + lo with |v - hi - lo| <= 2^-22 |v| and drops the lo x lo product (<= 2^-22 |w x|): at most 3 * 2^-22 of every |w x|.
Its fp32 accumulation runs through at most 18 chunk accumulations of 16-deep matrix products (288 = 32 x 9 contraction terms) plus the
bias, the residual, the ELU and the rounding (or 22-bit split) of the output: fewer than 28 roundings of 2^-24 of the running magnitude,
i.e. 7 * 2^-22.  So |y - ref| <= C_SPLIT * 2^-22 * (sum |w x| + |b|) with C_SPLIT = 10 for one layer; a residual block adds the first
layer's bound carried through the second layer's |w|.  Every case also stays within the bound of the matching toy-shape test."""
import numpy as np
import pytest
import torch

from oracle import stereo_oracle as O
from redtail_amd import capi
from layouts import from_il, from_split, pitched, to_il, to_split

pytestmark = pytest.mark.gpu

C_SPLIT = 10
EPS22 = 2.0 ** -22
HINT = capi.RT_HINT_THROUGHPUT
# C2's maps: the 1257 x 369 image, the half-resolution feature maps 629 x 185 (rows padded to 640), max disparity 48
IMG_H, IMG_W = 369, 1257
H, W, P, D = 185, 629, 640, 48
CORR_TOL = 2e-4 * D / 16                   # test_corr_softargmax_mfma's bound at D = 48


@pytest.fixture(scope="module")
def klib():
    return capi.KernelLib()


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(g, *shape):
    return torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)


def spread(g, x):
    """large activations next to tiny ones (as test_split_is_fp32_accurate_on_large_and_tiny_values)"""
    pick = torch.rand(x.shape, generator=g, device="cuda") < 0.5
    return x * torch.where(pick, torch.tensor(30.0, device="cuda"), torch.tensor(1e-3, device="cuda"))


def c64(a):
    return torch.as_tensor(a).detach().cpu().double()


def traced(capfd):
    """the [rt] lines written to stderr since the last call"""
    return [l for l in capfd.readouterr().err.splitlines() if l.startswith("[rt] ")]


def conv64(x, w, b, stride, pad):
    """fp64 result and the magnitude sum |w x| + |b| of the same convolution"""
    return O.conv2d(x, w, b, stride, pad), O.conv2d(x.abs(), w.abs(), b.abs(), stride, pad)


def check_bound(name, got, ref, bound):
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), name
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    assert (err <= bound).all(), (name, "first bad sample", worst, float(err[worst]), float(bound[worst]))
    print("%s: max err / bound %.3f" % (name, (err / bound).max()))
    return err


# ---- the tower block: 32 -> 32 -> 32, ELU / ELU, on interleaved and pre-split tensors (conv_rbs.hip.h, conv_rbd.hip.h) ---------------
# C2's eight blocks per tower run both towers in one launch (batch 2): the first reads the interleaved fp32 output of conv1 and writes
# the pre-split form, six read and write it, the last writes the interleaved fp32 tensor encoder2D_out reads.  Strips of S3RBSCfg::SW = 30
# columns (21 strips, the last one 29 columns wide), segments of 64 rows under the throughput hint (185 = 64 + 64 + 57).
@pytest.mark.parametrize("x_split,y_split,kernel", [(0, 1, "conv_s3rbs<1>"), (1, 1, "conv_s3rbd<1>"), (1, 0, "conv_s3rbd<0>")])
def test_c2_tower_block(klib, monkeypatch, capfd, x_split, y_split, kernel):
    monkeypatch.setenv("RT_CONV_TRACE", "1")
    g = gen(100 + 2 * x_split + y_split)
    c, batch = 32, 2
    x = spread(g, randn(g, batch, c, H, W))
    w1, b1 = randn(g, c, c, 3, 3) / np.sqrt(c * 9), randn(g, c)
    w2, b2 = randn(g, c, c, 3, 3) / np.sqrt(c * 9), randn(g, c)
    xp = pitched(x.cpu().numpy(), P)
    xs = to_split(xp)
    xv = from_split(xs)[..., :W] if x_split else x.cpu().numpy()          # the values the block computes on
    X, W1, B1, W2, B2 = c64(xv), c64(w1), c64(b1), c64(w2), c64(b2)
    t, mag1 = conv64(X, W1, B1, 1, 1)
    t = O.elu(t)
    y, mag2 = conv64(t, W2, B2, 1, 1)
    ref = O.elu(y + X).numpy()
    bound = C_SPLIT * EPS22 * (mag2 + X.abs() + O.conv2d(mag1, W2.abs(), None, 1, 1)).numpy()
    del t, y, mag1, mag2

    plan = klib.resblock_plan(w1.cpu().numpy(), b1.cpu().numpy(), w2.cpu().numpy(), b2.cpu().numpy(), c, c, H, W)
    plan.set_pitch(P, P)
    plan.set_layouts(1, 1, 1)
    plan.set_split(x_split, y_split)
    xin = torch.from_numpy(xs if x_split else to_il(xp, 4)).cuda()
    out = torch.full((batch, c // 8, H, P, 8) if y_split else (batch, c // 4, H, P, 4), float("nan"), device="cuda")
    traced(capfd)
    plan.enqueue(xin, out, xin, batch, hints=HINT)
    torch.cuda.synchronize()
    assert traced(capfd) == ["[rt] %s grid 63 x 1 x 2 seg 64" % kernel]
    plan.destroy()
    raw = out.cpu().numpy()
    assert np.isnan(raw[:, :, :, W:]).all(), "padding columns were written"
    got = (from_split(raw) if y_split else from_il(raw))[..., :W]
    err = check_bound(kernel, got, ref, bound)
    assert err.max() <= 2e-6 * max(1.0, np.abs(ref).max())                # test_split_resblock_presplit_tensors' bound


# ---- conv1 of both towers in one launch: 5x5 stride 2 on the 3-channel images, interleaved fp32 output (conv_s3_first_kernel<true>) ----
def test_c2_first_layer_twin_input(klib, monkeypatch, capfd):
    monkeypatch.setenv("RT_CONV_TRACE", "1")
    g = gen(200)
    left = torch.rand((1, 3, IMG_H, IMG_W), generator=g, device="cuda")
    right = torch.rand((1, 3, IMG_H, IMG_W), generator=g, device="cuda")
    w, b = randn(g, 32, 3, 5, 5) / np.sqrt(75), randn(g, 32)
    y, mag = conv64(torch.cat([c64(left), c64(right)]), c64(w), c64(b), 2, 2)
    ref, bound = O.elu(y).numpy(), (C_SPLIT * EPS22 * mag).numpy()
    plan = klib.conv2d_plan(w.cpu().numpy(), b.cpu().numpy(), 3, 32, IMG_H, IMG_W, 5, 2, 2, act=capi.RT_ACT_ELU)
    assert tuple(plan.out_dims[:3]) == (32, H, W)
    plan.set_pitch(0, P)
    plan.set_layouts(0, 1)
    out = torch.full((2, 8, H, P, 4), float("nan"), device="cuda")
    traced(capfd)
    plan.enqueue_twin_input(left, right, out, 1, hints=HINT)
    torch.cuda.synchronize()
    assert traced(capfd) == ["[rt] conv_s3_first<1> grid 940 x 1 x 2 twin 1"]
    plan.destroy()
    raw = from_il(out.cpu().numpy())
    assert np.isnan(raw[..., W:]).all(), "padding columns were written"
    err = check_bound("conv_s3_first<1>", raw[..., :W], ref, bound)
    assert err.max() <= 3e-6                                              # test_split_first_layer's bound


# ---- correlation + soft-argmax ----------------------------------------------------------------------------------------------------
def test_c2_corr_softargmax_into_the_ninth_group(klib, monkeypatch, capfd):
    """the engine's launch: interleaved encoder2D_out maps in, the map written as lane 0 of the ninth channel group of conv2D_1's input"""
    monkeypatch.setenv("RT_CONV_TRACE", "1")
    g = gen(300)
    l, r = randn(g, 1, 32, H, W) * 0.5, randn(g, 1, 32, H, W) * 0.5
    ref = O.softargmax(O.corr_cost_volume(c64(l), c64(r), D), False).numpy()
    lil = torch.from_numpy(to_il(pitched(l.cpu().numpy(), P), 4)).cuda()
    ril = torch.from_numpy(to_il(pitched(r.cpu().numpy(), P), 4)).cuda()
    buf = torch.full((1, 9, H, P, 4), float("nan"), device="cuda")
    traced(capfd)
    klib.corr_softargmax_il(lil, ril, buf[:, 8], 1, 32, H, W, D, False, P, P, out_bstride=9 * H * P * 4, out_slot=4)
    torch.cuda.synchronize()
    assert traced(capfd) == ["[rt] corr_softargmax_mfma<0,0> grid 925 slot 4"]
    got = buf.cpu().numpy()
    assert np.isnan(got[:, :8]).all() and np.isnan(got[:, 8, :, W:]).all(), "outside the map's slots was written"
    assert (got[:, 8, :, :W, 1:] == 0).all()
    check_bound("corr_softargmax_mfma<0,0>", got[:, 8, :, :W, 0], ref[:, 0], np.full(ref[:, 0].shape, CORR_TOL))


def range_edge_maps(g, big):
    """C2-sized maps whose channels 0-3 of the left and 4-7 of the right map hold values up to `big` at a quarter of the pixels, facing
    small nonzero values (|v| ~ 2e-5) in the other map: products of both sizes enter every correlation, which stays in the range where
    the soft-argmax is well conditioned"""
    l, r = randn(g, 1, 32, H, W) * 0.5, randn(g, 1, 32, H, W) * 0.5
    m = (torch.rand((1, 4, H, W), generator=g, device="cuda") < 0.25).float()
    l[:, 0:4] = m * big * (2 * torch.rand((1, 4, H, W), generator=g, device="cuda") - 1)
    l[:, 0, ::7, ::5] = big
    r[:, 0:4] = 2e-5 * randn(g, 1, 4, H, W)
    r[:, 4:8] = m * big * (2 * torch.rand((1, 4, H, W), generator=g, device="cuda") - 1)
    r[:, 5, ::5, ::7] = -big
    l[:, 4:8] = 2e-5 * randn(g, 1, 4, H, W)
    return l.contiguous(), r.contiguous()


def test_c2_corr_entries_inside_the_default_domain(klib, monkeypatch, capfd):
    """rt_corr_softargmax / rt_corr_cost_volume at C2's map size pick the 3-term fp16-split kernels; inputs up to 6e4 (inside the
    documented |x| < 65504) give an fp32-class result"""
    monkeypatch.setenv("RT_CONV_TRACE", "1")
    l, r = range_edge_maps(gen(400), 6.0e4)
    ref_cv = O.corr_cost_volume(c64(l), c64(r), D)
    ref = O.softargmax(ref_cv, False).numpy()
    out = torch.full((1, 1, H, W), float("nan"), device="cuda")
    traced(capfd)
    klib.corr_softargmax(l, r, out, 1, 32, H, W, D, False)
    torch.cuda.synchronize()
    assert traced(capfd) == ["[rt] corr_softargmax_mfma<0,1> grid 925 slot 1"]
    check_bound("corr_softargmax_mfma<0,1>", out.cpu().numpy(), ref, np.full(ref.shape, CORR_TOL))
    cv = torch.full((1, D, H, W), float("nan"), device="cuda")
    klib.corr_cost_volume(l, r, cv, 1, 32, H, W, D)
    torch.cuda.synchronize()
    assert traced(capfd) == ["[rt] corr_mfma_planar grid 928"]
    mag = O.corr_cost_volume(c64(l).abs(), c64(r).abs(), D).numpy()
    err = check_bound("corr_mfma_planar", c64(cv).numpy(), ref_cv.numpy(), C_SPLIT * EPS22 * mag + 1e-30)
    assert err.max() <= 5e-5                                              # test_corr_full_size's bound


@pytest.mark.parametrize("how", ["flags", "env"])
def test_c2_corr_entries_exact_beyond_fp16_range(klib, monkeypatch, capfd, how):
    """with RT_CONV_EXACT_FP32 -- the flag of rt_corr_softargmax_flags / rt_corr_cost_volume_flags, or the development knob -- inputs of
    magnitude 1e5 (outside the default path's domain) give the fp32 reference"""
    monkeypatch.setenv("RT_CONV_TRACE", "1")
    flags = capi.RT_CONV_EXACT_FP32 if how == "flags" else 0
    if how == "env":
        monkeypatch.setenv("RT_CONV_EXACT_FP32", "1")
    l, r = range_edge_maps(gen(500), 1.0e5)
    ref_cv = O.corr_cost_volume(c64(l), c64(r), D)
    ref = O.softargmax(ref_cv, False).numpy()
    out = torch.full((1, 1, H, W), float("nan"), device="cuda")
    traced(capfd)
    klib.corr_softargmax(l, r, out, 1, 32, H, W, D, False, flags=flags)
    torch.cuda.synchronize()
    assert traced(capfd) == ["[rt] corr_f32<12,1,0,0,f32> grid 5 x 47 x 1 d_base 0"]
    check_bound("corr_f32 fused", out.cpu().numpy(), ref, np.full(ref.shape, CORR_TOL))
    cv = torch.full((1, D, H, W), float("nan"), device="cuda")
    klib.corr_cost_volume(l, r, cv, 1, 32, H, W, D, flags=flags)
    torch.cuda.synchronize()
    assert traced(capfd) == ["[rt] corr_f32<12,0,0,0,f32> grid 5 x 47 x 1 d_base 0"]
    assert (c64(cv) - ref_cv).abs().max().item() <= 5e-5


# ---- the 2-D tail: conv_s3_kernel at every resolution, the transposed layers as four 2 x 2 phases, deconv3d_s2_small_kernel ------------
def c_split(k):
    """C_SPLIT for a contraction of k terms: 3 (operand split) + (ceil(k / 16) chunk accumulations + 10 other roundings) / 4"""
    return 3 + (-(-k // 16) + 10) / 4


C2_CONVS = [
    # layer, cin, cout, h, w, stride, transposed, batch, (x_il, y_il, r_il), residual, trace line
    ("conv2D_1", 33, 32, H, W, 1, False, 1, (1, 1, 0), False, "[rt] conv_s3<3,3,1,1,1,4,f32,f32> r0 grid 940 x 1 x 1 ks 1"),
    ("encoder2D_out", 32, 32, H, W, 1, False, 2, (1, 1, 0), False, "[rt] conv_s3<3,3,1,1,1,4,f32,f32> r0 grid 940 x 1 x 2 ks 1"),
    ("conv2D_3ds", 32, 64, H, W, 2, False, 1, (1, 1, 0), False, "[rt] conv_s3<3,3,2,1,1,4,f32,f32> r0 grid 240 x 2 x 1 ks 1"),
    ("conv2D_4", 64, 64, 93, 315, 1, False, 1, (1, 1, 0), False, "[rt] conv_s3<3,3,1,1,1,4,f32,f32> r0 grid 240 x 2 x 1 ks 1"),
    ("conv2D_6ds", 64, 128, 93, 315, 2, False, 1, (1, 1, 0), False, "[rt] conv_s3<3,3,2,1,1,4,f32,f32> r0 grid 60 x 4 x 1 ks 1"),
    ("conv2D_7", 128, 128, 47, 158, 1, False, 1, (1, 1, 0), False, "[rt] conv_s3<3,3,1,1,1,4,f32,f32> r0 grid 60 x 4 x 1 ks 1"),
    ("deconv2D_1", 128, 64, 47, 158, 2, True, 1, (1, 1, 1), True, "[rt] conv_s3<2,2,1,1,1,4,f32,f32> r1 grid 60 x 2 x 4 ks 1"),
    ("deconv2D_2", 64, 32, 93, 315, 2, True, 1, (1, 0, 1), True, "[rt] conv_s3<2,2,1,1,0,4,f32,f32> r1 grid 240 x 1 x 4 ks 1"),
]


def pad32(n):
    return (n + 31) // 32 * 32


@pytest.mark.parametrize("layer,cin,cout,h,w,stride,tr,batch,il,resid,line", C2_CONVS, ids=[c[0] for c in C2_CONVS])
def test_c2_tail_conv(klib, monkeypatch, capfd, layer, cin, cout, h, w, stride, tr, batch, il, resid, line):
    """ELU after every layer, the transposed ones with their skip tensor as residual (networks.cpp: createResNet18_2DNetwork); conv2D_1
    reads the 33-channel concatenation as 9 interleaved groups of 4 (the 36th-34th channels zero)"""
    monkeypatch.setenv("RT_CONV_TRACE", "1")
    g = gen(600 + len(layer) * 7 + cin)
    x_il, y_il, r_il = il
    x = randn(g, batch, cin, h, w)
    x = x * torch.where(torch.rand(x.shape, generator=g, device="cuda") < 0.5, torch.tensor(2.0, device="cuda"), torch.tensor(1e-3, device="cuda"))
    k_eff = cin * 9 / (4 if tr else 1)
    wt = randn(g, *((cin, cout, 3, 3) if tr else (cout, cin, 3, 3))) / np.sqrt(k_eff)
    b = randn(g, cout)
    X, Wt, B = c64(x), c64(wt), c64(b)
    if tr:
        y, mag = O.deconv2d(X, Wt, B, 2, 1), O.deconv2d(X.abs(), Wt.abs(), B.abs(), 2, 1)
    else:
        y, mag = conv64(X, Wt, B, stride, 1)
    ho, wo = y.shape[-2:]
    res = randn(g, batch, cout, ho, wo) if resid else None
    if resid:
        y, mag = y + c64(res), mag + c64(res).abs()
    ref, bound = O.elu(y).numpy(), (c_split(cin * 9) * EPS22 * mag).numpy()
    ip, op = pad32(w), pad32(wo)
    plan = klib.conv2d_plan(wt.cpu().numpy(), b.cpu().numpy(), cin, cout, h, w, 3, stride, 1, act=capi.RT_ACT_ELU, has_residual=resid,
                            transposed=tr)
    plan.set_pitch(ip, op)
    plan.set_layouts(x_il, y_il, r_il)
    cpad = (cin + 3) // 4 * 4
    xh = np.zeros((batch, cpad, h, ip), np.float32)
    xh[:, :cin] = pitched(x.cpu().numpy(), ip)
    if cpad != cin:
        plan.set_batch_strides(cpad * h * ip, 0, 0)
    xin = torch.from_numpy(to_il(xh, 4) if x_il else xh[:, :cin].copy()).cuda()
    rin = torch.from_numpy(to_il(pitched(res.cpu().numpy(), op), 4) if r_il else pitched(res.cpu().numpy(), op)).cuda() if resid else None
    out = torch.full((batch, cout // 4, ho, op, 4) if y_il else (batch, cout, ho, op), float("nan"), device="cuda")
    traced(capfd)
    plan.enqueue(xin, out, rin, batch, hints=HINT)
    torch.cuda.synchronize()
    assert traced(capfd) == [line]
    plan.destroy()
    raw = out.cpu().numpy()
    raw = from_il(raw) if y_il else raw
    assert np.isnan(raw[..., wo:]).all(), "padding columns were written"
    err = check_bound(layer, raw[..., :wo], ref, bound)
    assert err.max() <= 4e-7 * np.sqrt(cin * 9) + 2e-6, err.max()         # test_split_general's bound


def test_c2_last_transposed_layer(klib, monkeypatch, capfd):
    """deconv2D_3: 32 -> 1 channel, 629 x 185 -> 1257 x 369, sigmoid -- deconv3d_s2_small_kernel (fp32 fmaf chain of at most 4 taps x 32
    channels = 128 terms per output: 128 roundings of 2^-24 = 32 * 2^-22 of sum |w x| + |b|, two more for the bias and the sigmoid)"""
    monkeypatch.setenv("RT_CONV_TRACE", "1")
    g = gen(700)
    x = spread(g, randn(g, 1, 32, H, W)) / 10
    wt, b = randn(g, 32, 1, 3, 3) / np.sqrt(32 * 9 / 4), randn(g, 1)
    X, Wt, B = c64(x), c64(wt), c64(b)
    y, mag = O.deconv2d(X, Wt, B, 2, 1), O.deconv2d(X.abs(), Wt.abs(), B.abs(), 2, 1)
    assert tuple(y.shape[-2:]) == (IMG_H, IMG_W)
    ref, bound = torch.sigmoid(y).numpy(), (34 * EPS22 * mag).numpy()
    plan = klib.conv2d_plan(wt.cpu().numpy(), b.cpu().numpy(), 32, 1, H, W, 3, 2, 1, act=capi.RT_ACT_SIGMOID, transposed=True)
    plan.set_pitch(P, 0)
    out = torch.full((1, 1, IMG_H, IMG_W), float("nan"), device="cuda")
    traced(capfd)
    plan.enqueue(torch.from_numpy(pitched(x.cpu().numpy(), P)).cuda(), out, None, 1, hints=HINT)
    torch.cuda.synchronize()
    assert traced(capfd) == ["[rt] deconv3d_s2_small<1,0,f32,f32> grid 3 x 185 x 1"]
    plan.destroy()
    err = check_bound("deconv3d_s2_small<1,0,f32,f32>", out.cpu().numpy(), ref, bound)
    assert err.max() <= 5e-5                                              # test_deconv2d_full_size's bound


# ---- coverage: every launch of the C2 engine has a case above ---------------------------------------------------------------------
C2_TABLE = {"[rt] %s grid 63 x 1 x 2 seg 64" % k for k in ("conv_s3rbs<1>", "conv_s3rbd<1>", "conv_s3rbd<0>")} | {c[-1] for c in C2_CONVS} | {
    "[rt] conv_s3_first<1> grid 940 x 1 x 2 twin 1", "[rt] corr_softargmax_mfma<0,0> grid 925 slot 4",
    "[rt] deconv3d_s2_small<1,0,f32,f32> grid 3 x 185 x 1"}


def test_c2_engine_launches_are_all_in_the_table(monkeypatch, capfd):
    """the engine as bench.py times it (seeded synthetic weights, one stream per context, graph mode off), one batch under RT_CONV_TRACE:
    its distinct launches are exactly the table's -- a launch without an fp64 case above fails here"""
    import bench
    from redtail_amd import synth
    monkeypatch.setenv("RT_CONV_TRACE", "1")
    weights, _ = bench.load_weights(False)
    lib = capi.NetLib()
    net = lib.create("resnet18_2D", IMG_W, IMG_H, max_batch=1, weights=capi.pack_weights(weights, fp16=False), fp16_weights=False)
    net.set_streams(1)
    l, r = synth.synth_pair(IMG_H, IMG_W, 4321)
    left, right = torch.from_numpy(l[None]).cuda(), torch.from_numpy(r[None]).cuda()
    disp = torch.empty(1, 1, IMG_H, IMG_W, device="cuda")
    stream = bench.make_streams(lib.kernels, 1, torch.device("cuda"))[0]
    traced(capfd)
    net.execute(left, right, disp, 1, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    lines = set(traced(capfd))
    net.destroy()
    assert lines == C2_TABLE, ("launched without a case", sorted(lines - C2_TABLE), "cases the engine no longer launches", sorted(C2_TABLE - lines))
