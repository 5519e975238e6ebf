"""The first and the last layer of the 2-D network at the shapes where their gathers can go wrong.

conv_s3_first_kernel (conv_split.hip.h) reads the image in runs of 4 columns, one 16-byte load per channel: rows of a dense binding have an
odd pitch, so a run starts at any 4-byte boundary, and runs that cross an edge of the row take their elements one by one.
deconv3d_s2_small_kernel's 2-D sparse path (deconv3d_small.hip.h) loads a lane's own column only and takes column x + 1 from the lane to
its right: the last lane of a wave, the last lane of a workgroup and the last column of the image have no such lane.

Against fp64 with the bounds of the tests these kernels already have (test_timed_shapes.py::test_c2_last_transposed_layer,
test_split_parity.py::test_split_first_layer), on both backends; and, on the emulator, against the bytes the kernels produced before they
were restructured (tests/golden/edge_layers.npz, made by tests/golden/make_edge_layers.py from an emulator build of that commit): the new code
runs the same arithmetic in the same order."""
import os

import numpy as np
import pytest
import torch

from oracle import stereo_oracle as O
from redtail_amd import capi
from layouts import from_il, pitched

EPS22 = 2.0 ** -22
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_layers.npz")


class _Host:
    """the part of a backend run_last / run_first use, for a library opened outside pytest (tests/golden/make_edge_layers.py)"""

    def __init__(self, klib):
        self.klib = klib

    def dev(self, a):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).copy()

    def empty(self, shape):
        return np.full(shape, np.nan, dtype=np.float32)

    def host(self, t):
        return np.asarray(t)


def c64(a):
    return torch.from_numpy(np.asarray(a)).double()


# ---- last layer: 3x3 stride-2 transposed, cin -> 1 -------------------------------------------------------------------------------------
def run_last(backend, x, wt, b, act, pitch):
    """x (N, K, Hy, Wy) -> (N, 1, 2 Hy - 1, 2 Wy - 1); pitch = 0: dense input rows"""
    n, k, hy, wy = x.shape
    plan = backend.klib.conv2d_plan(wt, b, k, 1, hy, wy, 3, 2, 1, act=act, transposed=True)
    assert tuple(plan.out_dims[:3]) == (1, 2 * hy - 1, 2 * wy - 1)
    if pitch:
        plan.set_pitch(pitch, 0)
    y = backend.empty((n, 1, 2 * hy - 1, 2 * wy - 1))
    plan.enqueue(backend.dev(pitched(x, pitch) if pitch else x), y, None, n)
    out = backend.host(y).copy()
    plan.destroy()
    return out


def last_inputs(seed, k, hy, wy, batch=2):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((batch, k, hy, wy)).astype(np.float32)
    x *= np.where(rng.random(x.shape) < 0.5, np.float32(3.0), np.float32(1e-4))        # large next to tiny, as test_timed_shapes.spread
    wt = (rng.standard_normal((k, 1, 3, 3)) / np.sqrt(k * 9 / 4)).astype(np.float32)
    return x, wt, rng.standard_normal(1).astype(np.float32)


@pytest.mark.parametrize("k", [32, 5, 9])                 # four groups of 8 channels; the remainder loop only; one group + one
@pytest.mark.parametrize("wy", [63, 65, 257])             # a right neighbour outside the image, in the next wave, in the next workgroup
def test_last_layer_2d_against_fp64(backend, wy, k):
    """Hy = 3: row y + 1 of the last block row is outside; Wx = 2 Wy - 1 is odd: the last column has one phase.  fp32 fmaf chain of at
    most 4 taps x K channels: the bound of test_c2_last_transposed_layer (K <= 32)."""
    hy = 3
    x, wt, b = last_inputs(1000 + wy + k, k, hy, wy)
    X, Wt, B = c64(x), c64(wt), c64(b)
    y, mag = O.deconv2d(X, Wt, B, 2, 1), O.deconv2d(X.abs(), Wt.abs(), B.abs(), 2, 1)
    assert tuple(y.shape) == (2, 1, 2 * hy - 1, 2 * wy - 1)
    bound = (34 * EPS22 * mag).numpy()
    for act, ref in ((capi.RT_ACT_NONE, y.numpy()), (capi.RT_ACT_SIGMOID, torch.sigmoid(y).numpy())):
        for pitch in (0, (wy + 63) // 32 * 32):
            out = run_last(backend, x, wt, b, act, pitch)
            err = np.abs(out - ref)
            assert np.isfinite(out).all(), (act, pitch)
            worst = np.unravel_index(np.argmax(err / bound), err.shape)
            print("wy %d k %d act %d pitch %d: max err / bound %.3f" % (wy, k, act, pitch, (err / bound).max()))
            assert (err <= bound).all(), (act, pitch, "first bad sample", worst, float(err[worst]), float(bound[worst]))


# ---- first layer: 5x5 stride 2 on <= 3 channels, both towers through the twin-input entry ------------------------------------------------
def run_first(backend, left, right, wt, b, act, y_il, pad_to=32):
    """samples [0, n) from `left`, [n, 2n) from `right` (another allocation); returns the stored tensor as (2n, Cout, Ho, P) and Wo"""
    n, cin, h, w = left.shape
    cout = wt.shape[0]
    plan = backend.klib.conv2d_plan(wt, b, cin, cout, h, w, 5, 2, 2, act=act)
    _, ho, wo = plan.out_dims[:3]
    P = (wo + pad_to - 1) // pad_to * pad_to
    plan.set_pitch(0, P)
    if y_il:
        plan.set_layouts(0, 1)
    y = backend.empty((2 * n, cout // 4, ho, P, 4) if y_il else (2 * n, cout, ho, P))
    plan.enqueue_twin_input(backend.dev(left), backend.dev(right), y, n)
    out = backend.host(y).copy()
    plan.destroy()
    return (from_il(out) if y_il else out), wo


def first_inputs(seed, cin, cout, h, w):
    rng = np.random.default_rng(seed)
    left, right = (rng.standard_normal((1, cin, h, w)).astype(np.float32) for _ in range(2))
    wt = (rng.standard_normal((cout, cin, 5, 5)) / np.sqrt(cin * 25)).astype(np.float32)
    return left, right, wt, rng.standard_normal(cout).astype(np.float32)


@pytest.mark.parametrize("cin,h,w", [
    (3, 21, 133),       # dense rows of an odd width; three tile columns, the last one 3 pixels wide; a partial tile row
    (1, 5, 7),          # grey image smaller than a tile (and than a run's reach: every run crosses an edge)
])
def test_first_layer_against_fp64(backend, cin, h, w):
    left, right, wt, b = first_inputs(2000 + w, cin, 32, h, w)
    ref = O.elu(O.conv2d(torch.cat([c64(left), c64(right)]), c64(wt), c64(b), 2, 2)).numpy()
    outs = []
    for y_il in (0, 1):
        out, wo = run_first(backend, left, right, wt, b, capi.RT_ACT_ELU, y_il)
        assert out.shape[-1] > wo and np.isnan(out[..., wo:]).all(), "padding columns were written"
        outs.append(out[..., :wo])
    err = np.abs(outs[0] - ref).max()
    print("first layer %d x %d x %d: max err %.3g" % (cin, h, w, err))
    assert err <= 3e-6, err                                      # test_split_first_layer's bound
    assert outs[0].tobytes() == outs[1].tobytes()                # layouts change addressing only


# ---- the same bits as before the kernels were restructured ---------------------------------------------------------------------------
def golden_cases(backend):
    """one seeded case per kernel, activation none: inputs and what the given library makes of them"""
    x, wt, b = last_inputs(31, 9, 3, 65)
    out = dict(last_x=x, last_w=wt, last_b=b, last_y=run_last(backend, x, wt, b, capi.RT_ACT_NONE, 0))
    left, right, fw, fb = first_inputs(32, 3, 8, 5, 133)
    y, wo = run_first(backend, left, right, fw, fb, capi.RT_ACT_NONE, 1)
    out.update(first_left=left, first_right=right, first_w=fw, first_b=fb, first_y=np.ascontiguousarray(y[..., :wo]))
    return out


def test_same_bits_as_before(backend):
    """emulator: byte for byte; GPU: the fp64 bounds above (its bit-equality with the previous kernels is measured by
    tools/time_edge_layers.py, which runs both builds on the device)"""
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    last = run_last(backend, g["last_x"], g["last_w"], g["last_b"], capi.RT_ACT_NONE, 0)
    first, wo = run_first(backend, g["first_left"], g["first_right"], g["first_w"], g["first_b"], capi.RT_ACT_NONE, 1)
    first = first[..., :wo]
    assert last.shape == g["last_y"].shape and first.shape == g["first_y"].shape
    if backend.name == "emu":
        assert last.tobytes() == g["last_y"].tobytes()
        assert first.tobytes() == g["first_y"].tobytes()
    else:
        X, Wt, B = c64(g["last_x"]), c64(g["last_w"]), c64(g["last_b"])
        bound = (34 * EPS22 * O.deconv2d(X.abs(), Wt.abs(), B.abs(), 2, 1)).numpy()
        assert (np.abs(last - O.deconv2d(X, Wt, B, 2, 1).numpy()) <= bound).all()
        ref = O.conv2d(torch.cat([c64(g["first_left"]), c64(g["first_right"])]), c64(g["first_w"]), c64(g["first_b"]), 2, 2).numpy()
        assert np.abs(first - ref).max() <= 3e-6
