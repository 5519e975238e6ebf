"""The small ops around the convolutions in the forms the rest of the suite does not reach: fp16 storage, 2-byte-aligned pointers, buffers
longer than one sweep of a launcher's capped grid, every order of rt_permute4d, every (source, destination) pair of rt_convert_format,
and what rt_hash_buffer and rt_check_range compute.  Every reference is numpy on the host, in fp64 where anything is rounded; fp16 inputs
are generated as fp16, so the reference and the kernel see the same operands.  Each test runs on the SIMT emulator and, with -m gpu, on the
device."""
import functools
import itertools

import numpy as np
import pytest
import torch

from redtail_amd import capi
from redtail_amd.capi import RT_ACT_ELU, RT_ACT_NONE, RT_ACT_SIGMOID, RT_F16, RT_F32
from test_f16_storage import dev16, empty16, host
from test_ops_parity import T, near

GUARD = 16          # elements behind every destination that must stay NaN
F16_MAX = 65504.0
F16_TINY = 2.0 ** -24


# ---- buffers ---------------------------------------------------------------------------------------------------------------
def buf_at(backend, n, off, f16, data=None):
    """a NaN-filled device buffer and its view of `n` elements whose address is `off` elements past a 16-byte boundary (off = 0: aligned);
    at least `off` elements in front of the view and GUARD behind it.  Returns (whole, view, elements in front of the view)"""
    isz = 2 if f16 else 4
    whole = empty16(backend, (n + 40,)) if f16 else backend.empty((n + 40,))
    lead = off
    while (capi._ptr(whole) + lead * isz) % 16 != (off * isz) % 16:
        lead += 1
    assert lead + n + GUARD <= n + 40
    view = whole[lead:lead + n]
    assert capi._ptr(view) % 16 == (off * isz) % 16
    if data is not None:
        flat = np.ascontiguousarray(data).reshape(-1)
        assert flat.size == n and flat.dtype == (np.float16 if f16 else np.float32)
        if backend.name == "gpu":
            view.copy_(T(flat.copy()))           # (the shared inputs are read-only, which torch.from_numpy warns about)
        else:
            view[...] = flat
    return whole, view, lead


def read(backend, t, f16):
    """host copy as float32 (fp16 widens exactly: signs of zero, subnormals and NaN survive)"""
    return host(backend, t) if f16 else np.asarray(backend.host(t))


def result(backend, whole, lead, n, f16):
    """the view's content, after checking that nothing in front of it or in the guard behind it was written"""
    h = read(backend, whole, f16)
    assert np.isnan(h[:lead]).all(), "elements in front of the destination were written"
    assert np.isnan(h[lead + n:]).all(), "elements behind the destination were written"
    return h[lead:lead + n]


def upload(backend, a):
    a = np.ascontiguousarray(a)
    return dev16(backend, a) if a.dtype == np.float16 else backend.dev(a)


def ulp16(ref):
    """spacing of fp16 at the reference, at least the smallest subnormal"""
    with np.errstate(over="ignore", invalid="ignore"):
        u = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64)
    return np.maximum(np.where(np.isfinite(u), u, 32.0), F16_TINY)      # (np.spacing(65504) is inf: the binade's spacing is 32)


def close16(got, ref, extra, what=""):
    """fp16 result `got` (widened) against the fp64 reference: |got - ref| <= 0.5 ulp16(ref) + extra; NaN exactly where the reference has
    it; where the reference rounds to an infinity, that infinity.  Returns the largest (|got - ref| - extra) / ulp16(ref)"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN positions differ"
    with np.errstate(over="ignore", invalid="ignore"):
        r16 = ref.astype(np.float16).astype(np.float64)
    over = np.isinf(r16) & ~nan
    assert np.array_equal(got[over], r16[over]), "a result past the fp16 range is not that infinity"
    fin = ~nan & ~over
    if not fin.any():
        return 0.0
    err, u = np.abs(got[fin] - ref[fin]), ulp16(ref[fin])
    worst = float(((err - extra) / u).max())
    print("%s: max (|got - ref| - %g) / ulp16 = %.4f" % (what, extra, worst))
    assert (err <= 0.5 * u + extra).all(), "%s: %.4f ulp16 beyond the fp32 term" % (what, worst)
    return worst


def bits16(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.float16)).view(np.uint16)


def same16(got, want16):
    """fp16 result (widened) against expected fp16: NaN at the same places, the same bits everywhere else"""
    got, want16 = np.asarray(got).reshape(-1), np.asarray(want16).reshape(-1)
    assert want16.dtype == np.float16 and got.shape == want16.shape
    nan = np.isnan(want16)
    assert np.array_equal(np.isnan(got), nan), "NaN positions differ"
    assert np.array_equal(bits16(got)[~nan], want16.view(np.uint16)[~nan])


# ---- A. element-wise ---------------------------------------------------------------------------------------------------------
SWEEP_EW = 4096 * 256            # threads of ew_blocks' capped grid
#                  a block of special values: +-0, the smallest subnormal, +-65504, -20, +-inf, NaN; for add_act the pairs a + b with
#                  sums past 65504 (65504 + 16 = 65520 is the tie that rounds to inf), inf - inf, and NaN on either side
SPECIAL_A = np.array([0.0, -0.0, F16_TINY, -F16_TINY, F16_MAX, -F16_MAX, -20.0, np.inf, -np.inf, np.nan, F16_MAX, 60000.0, -F16_MAX, F16_MAX,
                      np.inf, np.inf, 1.0, -0.0, F16_MAX], np.float16)
SPECIAL_B = np.array([-0.0, -0.0, F16_TINY, F16_TINY, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, F16_MAX, 10000.0, -F16_MAX, 16.0,
                      -np.inf, np.inf, np.nan, 0.0, 8.0], np.float16)

EW_OPS = {      # name -> (activation, adds b)
    "elu": (RT_ACT_ELU, False), "sigmoid": (RT_ACT_SIGMOID, False), "add_none": (RT_ACT_NONE, True), "add_elu": (RT_ACT_ELU, True),
    "add_sigmoid": (RT_ACT_SIGMOID, True)}


@functools.lru_cache(maxsize=4)
def ew_inputs(n, f16):
    """3 N(0,1) in the tensor's own type, the special values at the front and (reversed) at the very end, where the ragged tail is"""
    rng = np.random.default_rng(n)
    dt = np.float16 if f16 else np.float32
    a, b = ((3 * rng.standard_normal(n, dtype=np.float32)).astype(dt) for _ in range(2))
    k = SPECIAL_A.size
    if n >= 2 * k:
        a[:k], b[:k] = SPECIAL_A, SPECIAL_B
        a[-k:], b[-k:] = SPECIAL_A[::-1], SPECIAL_B[::-1]
    a.flags.writeable = b.flags.writeable = False
    return a, b


def act64(v, act):
    """the formulas common.hip.h documents, in fp64: ELU as TensorFlow's x > 0 ? x : exp(x) - 1"""
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        if act == RT_ACT_ELU:
            return np.where(v > 0, v, np.exp(v) - 1.0)
        if act == RT_ACT_SIGMOID:
            return 1.0 / (1.0 + np.exp(-v))
    return v


def ew_reference(a, b, act, add):
    """fp64 on the operands as stored.  The sum of add_act is formed in fp32 first: that is the arithmetic the op documents (fp16 storage,
    fp32 math), and one IEEE addition has one result"""
    with np.errstate(all="ignore"):
        v = a.astype(np.float32) + b.astype(np.float32) if add else a.astype(np.float32)
    return v, act64(v, act)


def ew_launch(klib, op, a, b, y, n, dtype):
    act, add = EW_OPS[op]
    if add:
        klib.add_act(a, b, y, n, act, dtype)
    elif op == "elu":
        klib.elu(a, y, n, dtype)
    else:
        klib.activation(a, y, n, act, dtype)


def ew_check(op, got, a, b, f16):
    act, add = EW_OPS[op]
    v, ref = ew_reference(a, b, act, add)
    if act == RT_ACT_NONE:                       # exact: the fp32 sum, rounded once to the tensor's type
        with np.errstate(over="ignore"):
            want = v.astype(np.float16) if f16 else v
        if f16:
            same16(got, want)
        else:
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])
    elif f16:
        # 0.5 ulp16: the single rounding to fp16.  2e-7: two fp32 ulps of 1.0 for expf and the subtraction / the division.
        # Measured maximum of (|got - ref| - 2e-7) / ulp16, the same on the emulator and on the MI355X: elu 0.4995, sigmoid 0.4996,
        # add_elu 0.5000, add_sigmoid 0.4997
        close16(got, ref, 2e-7, op)
    else:
        nan = np.isnan(ref)                      # fp32: the bound of test_ops_parity.test_elementwise_sizes
        assert np.array_equal(np.isnan(got), nan)
        fin = np.isfinite(ref)
        assert np.array_equal(got[~fin & ~nan], ref[~fin & ~nan])
        assert np.abs(got[fin] - ref[fin]).max() <= 1e-6


EW_F16_CASES = [(1, 0), (7, 0), (8, 0), (9, 0), (1027, 0),          # 16-byte path (ew_f16_kernel<8, *>), with and without a tail
                (4099, 1), (70001, 3),                              # 2-byte alignment only: ew_f16_kernel<1, *>
                (SWEEP_EW * 8 + 1027, 0),                           # one element more than a sweep of the capped grid, and a ragged tail
                (SWEEP_EW + 5, 1)]                                  # a second sweep of the <1, *> kernels


@pytest.mark.parametrize("op", list(EW_OPS))
@pytest.mark.parametrize("n,off", EW_F16_CASES)
def test_elementwise_f16(backend, n, off, op):
    a, b = ew_inputs(n, True)
    _, da, _ = buf_at(backend, n, off, True, a)
    _, db, _ = buf_at(backend, n, off, True, b)
    whole, dy, lead = buf_at(backend, n, off, True)
    ew_launch(backend.klib, op, da, db, dy, n, RT_F16)
    ew_check(op, result(backend, whole, lead, n, True), a, b, True)


@pytest.mark.parametrize("op", list(EW_OPS))
@pytest.mark.parametrize("n,off", [(SWEEP_EW * 4 + 1027, 0), (SWEEP_EW + 5, 1)])
def test_elementwise_f32_past_one_sweep(backend, n, off, op):
    """the fp32 twins: ew_f32_kernel<4, *> and <1, *> with a second trip through their grid-stride loops"""
    a, b = ew_inputs(n, False)
    _, da, _ = buf_at(backend, n, off, False, a)
    _, db, _ = buf_at(backend, n, off, False, b)
    whole, dy, lead = buf_at(backend, n, off, False)
    ew_launch(backend.klib, op, da, db, dy, n, RT_F32)
    ew_check(op, result(backend, whole, lead, n, False), a, b, False)


@pytest.mark.parametrize("op", list(EW_OPS))
@pytest.mark.parametrize("n,off", [(1027, 0), (4099, 1)])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_elementwise_in_place(backend, f16, n, off, op):
    """y is a.  Every element is read and written by one lane, once: a lane that walked into another lane's elements would apply the
    activation to them a second time, which a separate destination cannot show"""
    a, b = ew_inputs(n, f16)
    whole, da, lead = buf_at(backend, n, off, f16, a)
    _, db, _ = buf_at(backend, n, off, f16, b)
    ew_launch(backend.klib, op, da, db, da, n, RT_F16 if f16 else RT_F32)
    ew_check(op, result(backend, whole, lead, n, f16), a, b, f16)


# ---- B. pad / slice / concat (copy_rows_kernel) ------------------------------------------------------------------------------------------
SWEEP_COPY = 2048 * 256          # threads per row of launch_copy_rows' capped grid


def values(shape, f16, seed=0):
    """random values with both signs of zero and an fp16 subnormal among them, in the tensor's type; no NaN (NaN marks unwritten elements)"""
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    x = (3 * rng.standard_normal(shape, dtype=np.float32)).astype(np.float16 if f16 else np.float32)
    flat = x.reshape(-1)
    flat[::97] = -0.0
    flat[1::101] = F16_TINY
    return x


def exact(got, want, f16):
    """bit equality of a result without NaN"""
    near(np.asarray(got).reshape(-1), np.asarray(want, np.float32).reshape(-1), 0)
    if f16:
        same16(got, np.ascontiguousarray(want).reshape(-1))
    else:
        assert np.array_equal(np.asarray(got, np.float32).reshape(-1).view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32))


@pytest.mark.parametrize("inner", [7, 165])
def test_pad_slice_concat_f16(backend, inner):
    """odd row lengths: every row but the first starts on a 2-byte boundary only"""
    k, N, D = backend.klib, 2, 4
    x = values((N, D, inner), True)
    dx = upload(backend, x)
    for pad_end in (1, 2):
        n = N * (D + pad_end) * inner
        whole, dy, lead = buf_at(backend, n, 0, True)
        k.pad_d(dx, dy, N, D, inner, pad_end, RT_F16)
        want = np.zeros((N, D + pad_end, inner), np.float16)          # the padding is +0
        want[:, :D] = x
        exact(result(backend, whole, lead, n, True), want, True)
    for start, end in ((0, 2), (1, 3), (D - 1, D)):
        n = N * (end - start) * inner
        whole, dy, lead = buf_at(backend, n, 0, True)
        k.slice_d(dx, dy, N, D, inner, start, end, RT_F16)
        exact(result(backend, whole, lead, n, True), x[:, start:end], True)
    for c_off in (1, 3):                                              # into the middle of a wider buffer: the other channels stay NaN
        Ctot = D + 4
        n = N * Ctot * inner
        whole, dy, lead = buf_at(backend, n, 0, True)
        k.concat_channels(dx, dy, N, D, Ctot, c_off, inner, RT_F16)
        got = result(backend, whole, lead, n, True).reshape(N, Ctot, inner)
        exact(got[:, c_off:c_off + D], x, True)
        assert np.isnan(got[:, :c_off]).all() and np.isnan(got[:, c_off + D:]).all()


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_pad_row_past_one_sweep(backend, f16):
    """rows of 2048 * 256 + 77 elements and their zero tail: a third trip through copy_rows_kernel's loop, which ends inside the tail"""
    N, D, inner = 2, 5, (SWEEP_COPY + 77) // 5
    assert D * inner == SWEEP_COPY + 77
    x = values((N, D, inner), f16)
    n = N * (D + 1) * inner
    whole, dy, lead = buf_at(backend, n, 0, f16)
    backend.klib.pad_d(upload(backend, x), dy, N, D, inner, 1, RT_F16 if f16 else RT_F32)
    want = np.zeros((N, D + 1, inner), x.dtype)
    want[:, :D] = x
    exact(result(backend, whole, lead, n, f16), want, f16)


# ---- C. rt_permute4d ------------------------------------------------------------------------------------------------------------------
ORDERS = list(itertools.permutations(range(4)))
PERM_DIMS = [(2, 3, 4, 5), (3, 2, 5, 8), (2, 3, 4, 16)]
PERM_U = 256 * 8                 # elements (or 16-byte units) per block of permute_runs_kernel
SWEEP_PERM = 4096 * 256          # threads per sample of the generic kernel's capped grid


def permute_kernel(dims, order, f16, aligned):
    """which kernel rt_permute4d's launcher takes (rt_capi.hip): there is no trace line for it, so the choice follows from the arguments"""
    if order[3] != 3:
        return "permute4d"
    isz = 2 if f16 else 4
    inner = dims[2] * dims[3] if order[2] == 2 else dims[3]
    v16 = aligned and inner * isz % 16 == 0 and int(np.prod(dims)) * isz % 16 == 0
    return "runs16" if v16 else "runs"


def run_permute(backend, x, dims, order, f16, off, batch=2):
    n = x.size
    _, dx, _ = buf_at(backend, n, off, f16, x)
    whole, dy, lead = buf_at(backend, n, off, f16)
    backend.klib.permute4d(dx, dy, batch, dims, order, RT_F16 if f16 else RT_F32)
    want = np.ascontiguousarray(np.transpose(x, (0,) + tuple(1 + o for o in order)))
    exact(result(backend, whole, lead, n, f16), want, f16)


def test_permute_cases_reach_every_kernel():
    for f16 in (False, True):
        took = {permute_kernel(d, o, f16, True) for d in PERM_DIMS for o in ORDERS}
        assert took == {"permute4d", "runs", "runs16"}, took
        # one element off the 16-byte boundary: the scalar runs kernel wherever the aligned call took the 16-byte one
        assert {permute_kernel(d, o, f16, False) for d in PERM_DIMS for o in ORDERS} == {"permute4d", "runs"}


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "one_element_off"])
@pytest.mark.parametrize("dims", PERM_DIMS)
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_permute_all_orders(backend, f16, dims, off):
    """all 24 orders; every element has its own value (integers below 2048 are exact in fp16)"""
    total = 2 * int(np.prod(dims))
    assert total <= 2048
    x = np.arange(total, dtype=np.float32).reshape((2,) + dims).astype(np.float16 if f16 else np.float32)
    for order in ORDERS:
        run_permute(backend, x, dims, order, f16, off)


@pytest.mark.parametrize("f16,d3", [(False, 8200), (True, 16400),        # 2050 16-byte units a run: two chunks, the second nearly empty
                                    (False, 15600), (True, 31200),       # 3900 units: the second chunk is needed from 2048 on, not from 1792
                                    (False, 3999), (True, 3999)])        # the scalar kernel with two chunks, odd run length
def test_permute_runs_of_several_chunks(backend, f16, d3):
    dims, order = (2, 3, 1, d3), (1, 0, 2, 3)
    units = d3 // ((8 if f16 else 4) if permute_kernel(dims, order, f16, True) == "runs16" else 1)
    assert PERM_U < units <= 2 * PERM_U
    run_permute(backend, values((2,) + dims, f16), dims, order, f16, 0)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_permute_generic_past_one_sweep(backend, f16):
    dims, order = (3, 5, 7, 10007), (3, 0, 1, 2)
    assert int(np.prod(dims)) > SWEEP_PERM and permute_kernel(dims, order, f16, True) == "permute4d"
    run_permute(backend, values((1,) + dims, f16), dims, order, f16, 0, batch=1)


# ---- D. rt_convert_format ------------------------------------------------------------------------------------------------------------------
KIND_F32, KIND_F16, KIND_NC2HW2 = 0, 1, 2


def pack_nc2hw2(x16, spare):
    """(N, C, inner) fp16 -> (N, ceil(C / 2), inner, 2): channels (2i, 2i + 1) of a pixel side by side, `spare` behind an odd C"""
    n, c, inner = x16.shape
    cp = (c + 1) // 2
    full = np.full((n, 2 * cp, inner), spare, np.float16)
    full[:, :c] = x16
    return np.ascontiguousarray(full.reshape(n, cp, 2, inner).transpose(0, 1, 3, 2))


def cvt_source(shape, seed):
    """fp32 100 N(0,1) with, in every row: 65519.9 (-> 65504), 65520 (the tie, -> inf), 1e-8 (-> 0), 3e-6 (-> an fp16 subnormal), their
    negatives, -0 and NaN"""
    x = (100 * np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)).astype(np.float32)
    edge = np.array([65519.9, 65520.0, 1e-8, 3e-6, -0.0, np.nan, -65519.9, -65520.0, -1e-8, -3e-6], np.float32)
    x[..., 3:3 + edge.size] = edge
    with np.errstate(over="ignore"):
        e16 = edge.astype(np.float16)
    assert e16[0] == F16_MAX and np.isinf(e16[1]) and e16[2] == 0 and 0 < e16[3] < 2.0 ** -14 and np.signbit(e16[4])
    return x


def cvt_forms(x):
    """the source in each kind (NaN in the spare half of NC2HW2), and what each kind holds after a conversion from that kind"""
    with np.errstate(over="ignore"):
        x16 = x.astype(np.float16)               # numpy rounds to nearest even, like the conversion instruction
    src = {KIND_F32: x, KIND_F16: x16, KIND_NC2HW2: pack_nc2hw2(x16, np.nan)}
    want = {}
    for sk in src:                               # (a value that went through fp16 once converts again without change)
        want[sk] = {KIND_F32: x if sk == KIND_F32 else x16.astype(np.float32), KIND_F16: x16, KIND_NC2HW2: pack_nc2hw2(x16, 0.0)}
    return src, want


def cvt_run(backend, src, batch, C, inner, sk, dk, want):
    n = want.size
    f16 = dk != KIND_F32
    whole, dy, lead = buf_at(backend, n, 0, f16)
    backend.klib.convert_format(src, dy, batch, C, inner, sk, dk)
    got = result(backend, whole, lead, n, f16)
    if f16:
        same16(got, want)
    else:
        w = want.reshape(-1)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got.view(np.uint32)[~nan], w.view(np.uint32)[~nan])
    return dy


@pytest.mark.parametrize("C", [1, 2, 5])
def test_convert_format_all_pairs(backend, C):
    """the nine pairs, identities included.  Odd C: the spare half of the last NC2HW2 slot is written as +0 over the NaN that was there, and a
    NaN in the spare half of a source appears nowhere in the result (NaN positions are compared)"""
    batch, inner = 2, 37
    src, want = cvt_forms(cvt_source((batch, C, inner), C))
    for sk in src:
        dsrc = upload(backend, src[sk])
        for dk in (KIND_F32, KIND_F16, KIND_NC2HW2):
            cvt_run(backend, dsrc, batch, C, inner, sk, dk, want[sk][dk])


def test_convert_format_past_one_sweep(backend):
    """rows longer than the capped grid: fp32 -> NC2HW2 (odd C) -> fp32 gives the source rounded to fp16"""
    batch, C, inner = 1, 3, 4096 * 256 + 9
    src, want = cvt_forms(cvt_source((batch, C, inner), 7))
    packed = cvt_run(backend, upload(backend, src[KIND_F32]), batch, C, inner, KIND_F32, KIND_NC2HW2, want[KIND_F32][KIND_NC2HW2])
    cvt_run(backend, packed, batch, C, inner, KIND_NC2HW2, KIND_F32, want[KIND_NC2HW2][KIND_F32])


def test_convert_format_bad_arguments(backend):
    x = backend.dev(np.zeros(8, np.float32))
    with pytest.raises(capi.RtError):
        backend.klib.convert_format(x, x, 1, 1, 8, 0, 3)
    with pytest.raises(capi.RtError):
        backend.klib.convert_format(x, x, 1, 0, 8, 0, 1)


# ---- E. rt_hash_buffer ------------------------------------------------------------------------------------------------------------------
SWEEP_HASH = 1024 * 256          # threads of the capped grid; the launcher sizes it at 8 words a thread


def hash_ref(words):
    """the function hash_words_kernel's comment defines, modulo 2^64: sum over i of (v ^ v >> 29) * 0xbf58476d1ce4e5b9 with
    v = (word_i + 0x9e3779b97f4a7c15) * (2 i + 1)"""
    w = np.asarray(words, np.uint32).astype(np.uint64)
    i = np.arange(w.size, dtype=np.uint64)
    v = (w + np.uint64(0x9e3779b97f4a7c15)) * (np.uint64(2) * i + np.uint64(1))
    v ^= v >> np.uint64(29)
    return int((v * np.uint64(0xbf58476d1ce4e5b9)).sum(dtype=np.uint64))


def hash_dev(backend, words):
    w = np.ascontiguousarray(words, np.uint32)
    d = torch.from_numpy(w.view(np.int32)).cuda() if backend.name == "gpu" else w.copy()
    return backend.klib.hash_buffer(d, 4 * w.size)


def test_hash_reference_is_the_documented_function():
    """the numpy restatement against plain Python integers"""
    words = [0, 1, 0xffffffff, 0x12345678, 7]
    h = 0
    for i, w in enumerate(words):
        v = ((w + 0x9e3779b97f4a7c15) * (2 * i + 1)) % 2 ** 64
        v ^= v >> 29
        h = (h + v * 0xbf58476d1ce4e5b9) % 2 ** 64
    assert hash_ref(words) == h


@pytest.mark.parametrize("words", [1, 5, 2049, 70001, 1024 * 2048 + 333])
def test_hash_buffer_value(backend, words):
    w = np.random.default_rng(words).integers(0, 2 ** 32, words, dtype=np.uint64).astype(np.uint32)
    assert hash_dev(backend, w) == hash_ref(w)


def test_hash_buffer_of_zeros(backend):
    w = np.zeros(2049, np.uint32)
    got = hash_dev(backend, w)
    assert got == hash_ref(w) and got != 0


def test_hash_buffer_sensitivity(backend):
    """one flipped bit, wherever it is, and two swapped words change the value (and the value stays the documented one)"""
    n = 1024 * 2048 + 333
    for words, places in ((2049, (0, 2048)), (n, (0, 1024 * 2048 + 1, n - 1))):
        w = np.random.default_rng(5).integers(0, 2 ** 32, words, dtype=np.uint64).astype(np.uint32)
        base = hash_dev(backend, w)
        assert base == hash_ref(w)
        seen = {base}
        for at in places:
            for bit in (0, 31):
                m = w.copy()
                m[at] ^= np.uint32(1 << bit)
                got = hash_dev(backend, m)
                assert got == hash_ref(m) and got not in seen, (words, at, bit)
                seen.add(got)
        m = w.copy()
        m[[3, words - 2]] = m[[words - 2, 3]]
        assert m[3] != w[3]
        got = hash_dev(backend, m)
        assert got == hash_ref(m) and got not in seen


def test_hash_buffer_sizes(backend):
    x = backend.dev(np.ones(4, np.float32))
    assert backend.klib.hash_buffer(x, 0) == 0
    with pytest.raises(capi.RtError):
        backend.klib.hash_buffer(x, 6)


# ---- F. rt_check_range ------------------------------------------------------------------------------------------------------------------
SWEEP_RANGE = 2048 * 256


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_check_range_forms(backend, f16):
    k = backend.klib
    dt, dtype = (np.float16, RT_F16) if f16 else (np.float32, RT_F32)
    limit = dt(F16_MAX)
    below = np.nextafter(limit, dt(0))                        # the largest value of the tensor's type under the limit
    assert below < limit and below.dtype == dt
    rows, valid, pitch = 3, 8, 10
    x = np.zeros((rows, pitch), dt)
    x[:, :valid] = np.arange(rows * valid).reshape(rows, valid)
    x[:, valid] = np.nan                                      # the padding is not looked at
    x[:, valid + 1] = np.inf
    x[1, 3] = -1000.5                                         # max |x| comes from a negative element

    def run(a):
        return k.check_range(upload(backend, a), rows, valid, pitch, dtype, float(limit))

    assert run(x) == (1000.5, 0)
    y = x.copy()
    y[2, 7] = below                                           # just under the limit: not counted
    y[0, 0] = -below
    assert run(y) == (float(below), 0)
    y[2, 6] = limit                                           # the test is >=
    assert run(y) == (float(limit), 1)
    y[0, 1] = -limit
    assert run(y) == (float(limit), 2)
    for bad in (-np.inf, np.inf, np.nan):                     # non-finite: a violation, and max |x| is +inf (what the kernel documents)
        z = x.copy()
        z[1, 0] = bad
        assert run(z) == (float("inf"), 1)
        z[2, 5] = limit
        assert run(z) == (float("inf"), 2)
    d = upload(backend, x)
    assert k.check_range(d, 0, valid, pitch, dtype, float(limit)) == (0.0, 0)
    assert k.check_range(d, rows, 0, pitch, dtype, float(limit)) == (0.0, 0)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_check_range_past_one_sweep(backend, f16):
    """2048 * 256 + 99 elements, the only violation in the last one"""
    n = SWEEP_RANGE + 99
    x = values((n,), f16)
    x[5] = -123.0
    top = float(np.abs(x.astype(np.float64)).max())
    d = upload(backend, x)
    dtype = RT_F16 if f16 else RT_F32
    assert backend.klib.check_range(d, 1, n, n, dtype, 1000.0) == (top, 0)
    x[-1] = -1000.0
    assert backend.klib.check_range(upload(backend, x), 1, n, n, dtype, 1000.0) == (1000.0, 1)
    assert backend.klib.check_range(upload(backend, x), 1, n - 1, n, dtype, 1000.0) == (top, 0)


# ---- G. rt_softargmax, fp16 ------------------------------------------------------------------------------------------------------------------
def softargmax64(vol, is_min):
    x = vol.astype(np.float64)
    x = -x if is_min else x
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return (p * np.arange(x.shape[1], dtype=np.float64)[None, :, None, None]).sum(axis=1)


def run_softargmax16(backend, vol, is_min):
    n, D, H, W = vol.shape
    whole, out, lead = buf_at(backend, n * H * W, 0, True)
    backend.klib.softargmax(upload(backend, vol), out, n, D, H, W, is_min, dtype=RT_F16)
    got = result(backend, whole, lead, n * H * W, True)
    # 0.5 ulp16: the rounding of the result.  1e-5 max(D, 8): the fp32 bound of test_ops_parity.test_softargmax_random.
    # Measured maximum of (|got - ref| - that) / ulp16: 0.479 on the emulator and on the MI355X
    close16(got, softargmax64(vol, is_min), 1e-5 * max(D, 8), "softargmax D=%d" % D)


@pytest.mark.parametrize("scale", [3.0, 3000.0])
@pytest.mark.parametrize("is_min", [False, True], ids=["max", "min"])
@pytest.mark.parametrize("D", [1, 7, 8, 9, 136])
def test_softargmax_f16_forms(backend, D, is_min, scale):
    """scale 3000: inputs near the end of the fp16 range, where the online softmax's running maximum jumps by thousands between chunks"""
    rng = np.random.default_rng(D)
    vol = (scale * rng.standard_normal((2, D, 3, 67), dtype=np.float32)).astype(np.float16)
    assert np.isfinite(vol).all()
    run_softargmax16(backend, vol, is_min)


@pytest.mark.parametrize("hw", [257, 513])
def test_softargmax_f16_past_one_block(backend, hw):
    """one lane past a block edge"""
    vol = (3 * np.random.default_rng(hw).standard_normal((2, 9, 1, hw), dtype=np.float32)).astype(np.float16)
    run_softargmax16(backend, vol, False)
    run_softargmax16(backend, vol, True)
