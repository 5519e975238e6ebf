"""Which kernel a plan launches: one small plan per decision of the conv enqueue (rt_capi.hip: enqueue_conv and its launchers), enqueued once
under RT_CONV_TRACE, the [rt] lines compared with the list recorded for the case.  Values are other tests' business (test_conv_parity,
test_split_parity, test_f16_storage, test_deconv3d_half2, test_conv3d_depth_walk, test_wino_parity): the tensors here are zeros, the
weights seeded noise.  The emulator reports 256 compute units, as the MI355X does, so one list serves both backends.

Shapes: a few rows by 32-70 columns, <= 64 channels, depth <= 7 -- except where a case has to sit on a threshold of the launch heuristics
(the 120-workgroup rule of the tower block: one-pixel images in batches of 119 and 120, some seven seconds each on the emulator; the 18
depth blocks that make two segments of the last transposed layer's walk).  Not covered: the tower block under the hint with fewer than 120
workgroups of 64 rows but 120 of 32 -- that takes 33 rows x 60 samples, 40 s on the emulator; the 119-sample cases fall through the same
comparison."""
import numpy as np
import pytest

from redtail_amd import capi

F16, F32, ELU, NONE = capi.RT_F16, capi.RT_F32, capi.RT_ACT_ELU, capi.RT_ACT_NONE
HINT = capi.RT_HINT_THROUGHPUT
EXACT = capi.RT_CONV_EXACT_FP32


def rnd(*shape, f16=False):
    a = np.random.RandomState(sum(shape)).standard_normal(shape).astype(np.float32) * np.float32(0.05)
    return np.ascontiguousarray(a.astype(np.float16)) if f16 else a


def buf(b, n, f16=False, fill=0.0):
    """n elements on the backend's device"""
    a = np.full(int(n), fill, np.float16 if f16 else np.float32)
    if b.name == "gpu":
        import torch
        return torch.from_numpy(a).cuda()
    return a


def host(b, t):
    if b.name == "gpu":
        b.torch.cuda.synchronize()
        return t.float().cpu().numpy()
    return np.asarray(t).astype(np.float32)


def nout(plan, n):
    return n * int(np.prod(plan.out_dims))


# ---- plans ------------------------------------------------------------------------------------------------------------------------------
def conv2d(b, cin, cout, h, w, k=3, stride=1, tr=False, resid=False, flags=0, act=ELU, pitch=None):
    """pitch = (input, output) row pitch in elements, 0 = dense; the fp16 forms run on rows of 64 as in test_f16_storage"""
    wt = rnd(*((cin, cout, k, k) if tr else (cout, cin, k, k)))
    plan = b.klib.conv2d_plan(wt, rnd(cout), cin, cout, h, w, k, stride, 1 if tr else k // 2, act=act, has_residual=resid, transposed=tr, flags=flags)
    ip, op = pitch or (0, 0)
    if pitch:
        plan.set_pitch(ip, op)
    co, ho, wo = plan.out_dims[:3]
    plan.x_elems, plan.y_elems = cin * h * (ip or w), co * ho * (op or wo)          # per sample
    return plan


def run2d(b, plan, n=1, x16=False, y16=False, resid=False, hints=0, twin=False):
    """interleaved tensors hold the same number of elements as planar ones (channel counts here are whole groups)"""
    x, y = buf(b, n * plan.x_elems, x16), buf(b, (2 * n if twin else n) * plan.y_elems, y16, np.nan)
    if twin:
        plan.enqueue_twin_input(x, buf(b, n * plan.x_elems, x16), y, n, hints=hints)
    else:
        plan.enqueue(x, y, buf(b, n * plan.y_elems, y16) if resid else None, n, hints=hints)
    out = host(b, y)
    plan.destroy()
    return out


def deconv3d(b, K, C, ydims, dfull, dkeep, pad_d, f16, skip=False, cdhw=True, act=NONE):
    """Conv3DTranspose 3x3x3 stride 2 from (K, Dy, Hy, Wy) to (dkeep, C, 2 Hy - 1, 2 Wy - 1); returns plan, input and output elements per sample"""
    dy, hy, wy = ydims
    hx, wx = 2 * hy - 1, 2 * wy - 1
    ps = (pad_d, 1, 1)
    plan = b.klib.conv3d_plan(rnd(K, 3, C, 3, 3, f16=f16), rnd(C, f16=f16), C, K, (dfull, hx, wx), (3, 3, 3), (2, 2, 2), ps, ps, act=act, out_dchw=cdhw,
                              has_residual=skip, dtype=F16 if f16 else F32, transposed_in_dims=ydims, out_depth=dkeep)
    return plan, K * dy * hy * wy, C * dkeep * hx * wx


def run_last_deconv3d(b, K, C, ydims, dfull, dkeep, pad_d, f16, il=False, softarg=0, n=2):
    plan, nx, ny = deconv3d(b, K, C, ydims, dfull, dkeep, pad_d, f16, cdhw=False)
    if f16:
        plan.set_io_types(F16, F32)
    if il:
        plan.set_layouts(1, 0, 0)
    if softarg:
        plan.set_softarg(softarg)
    y = buf(b, n * ny, False, np.nan)            # (the soft-argmax map is smaller than the volume)
    plan.enqueue(buf(b, n * nx, f16), y, None, n)
    host(b, y)
    plan.destroy()


def run_deconv3d(b, K, C, ydims, dfull, dkeep, pad_d, f16, layouts=None, skip=True, n=2):
    plan, nx, ny = deconv3d(b, K, C, ydims, dfull, dkeep, pad_d, f16, skip=skip, act=ELU)
    if f16:
        plan.set_io_types(F16, F16)
    if layouts:
        plan.set_layouts(*layouts)
    y = buf(b, n * ny, f16, np.nan)
    plan.enqueue(buf(b, n * nx, f16), y, buf(b, n * ny, f16) if skip else None, n)
    host(b, y)
    plan.destroy()


def run_conv3d(b, c, k, d, h, w, f16, il=False, resid=False, act=ELU, stride=1, x16=None, cm=False, n=2):
    """Conv3D 3x3x3; f16 + il: between channel-interleaved fp16 tensors (D, C/8, H, W, 8)"""
    plan = b.klib.conv3d_plan(rnd(k, 3, c, 3, 3, f16=f16), rnd(k, f16=f16), c, k, (d, h, w), (3, 3, 3), (stride,) * 3, (1, 1, 1), (1, 1, 1), act=act,
                              out_dchw=not cm, has_residual=resid, dtype=F16 if f16 else F32)
    x16 = f16 if x16 is None else x16
    if f16:
        plan.set_io_types(F16 if x16 else F32, F16)
    if il:
        plan.set_layouts(1, 1, 1 if resid else 0)
    y = buf(b, nout(plan, n), f16, np.nan)
    plan.enqueue(buf(b, n * d * c * h * w, x16), y, buf(b, nout(plan, n), f16) if resid else None, n)
    host(b, y)
    plan.destroy()


def run_block(b, h, w, n, split=None, f16=False, hints=0, c=32, cmid=32, il=True, pitch=0):
    """the fused residual block; split = (x_split, y_split): pre-split tensors (C/8, H, W, [8 hi | 8 lo] fp16) -- as many bytes as fp32 ones"""
    plan = b.klib.resblock_plan(rnd(cmid, c, 3, 3), rnd(cmid), rnd(c, cmid, 3, 3), rnd(c), c, cmid, h, w)
    if pitch:
        plan.set_pitch(pitch, pitch)
    if f16:
        plan.set_io_types(F16, F16)
    if il:
        plan.set_layouts(1, 1, 1)
    if split:
        plan.set_split(*split)
    x, y = buf(b, n * c * h * (pitch or w), f16), buf(b, n * c * h * (pitch or w), f16, np.nan)
    plan.enqueue(x, y, x, n, hints=hints)
    host(b, y)
    plan.destroy()


def finite(out):
    assert np.isfinite(out).all()


# ---- the cases: name -> (environment, needs the experimental families, what to run) ------------------------------------------------------
SMALL = (32, 1, (3, 4, 19), 7, 6, 0)             # the last Conv3DTranspose of the 3-D models: 32 channels -> 1, the surplus slice dropped
DEEP = (32, 1, (17, 3, 21), 35, 34, 0)           # 18 depth blocks
DECONV = (16, 8, (3, 4, 19), 7, 6, 0)            # NVSmall's decoder pattern
DW = {"RT_F16_DW": "1"}
CASES = {
    # deconv3d_s2_small and its interleaved-input forms
    "small_2d_f32": ({}, 0, lambda b: run2d(b, conv2d(b, 32, 1, 5, 33, tr=True, stride=2))),
    "small_2d_f16": ({}, 0, lambda b: run2d(b, io(conv2d(b, 32, 1, 5, 33, tr=True, stride=2, pitch=(64, 128)), F16, F16), x16=True, y16=True)),
    "small_3d_f32": ({}, 0, lambda b: run_last_deconv3d(b, *SMALL, f16=False)),
    "small_3d_f16_in": ({}, 0, lambda b: run_last_deconv3d(b, *SMALL, f16=True)),
    "small_3d_two_channels": ({}, 0, lambda b: run_last_deconv3d(b, 64, 2, (2, 3, 9), 5, 4, 0, f16=False)),
    "small_il": ({"RT_SMALL_IL_WALK": "0"}, 0, lambda b: run_last_deconv3d(b, *SMALL, f16=True, il=True)),
    "small_il_64_channels": ({}, 0, lambda b: run_last_deconv3d(b, 64, 2, (2, 3, 9), 5, 4, 0, f16=True, il=True)),
    "small_il4": ({}, 0, lambda b: run_last_deconv3d(b, *SMALL, f16=False, il=True)),
    "small_ilw_one_segment": ({}, 0, lambda b: run_last_deconv3d(b, *SMALL, f16=True, il=True)),
    "small_ilw_two_segments": ({}, 0, lambda b: run_last_deconv3d(b, *DEEP, f16=True, il=True)),
    "small_ilw_softargmax": ({}, 0, lambda b: run_last_deconv3d(b, *SMALL, f16=True, il=True, softarg=1)),
    "small_ilw_softargmin": ({}, 0, lambda b: run_last_deconv3d(b, *DEEP, f16=True, il=True, softarg=2)),
    # deconv_s3p: fp32 tensors, one launch per depth class
    "deconv_s3p_planar": ({}, 0, lambda b: run_deconv3d(b, *DECONV, f16=False)),
    "deconv_s3p_interleaved_out": ({}, 0, lambda b: run_deconv3d(b, *DECONV, f16=False, layouts=(0, 1, 1))),
    # deconv_f16p / deconv_f16pw
    "deconv_f16p": ({"RT_F16P_WALK": "0"}, 0, lambda b: run_deconv3d(b, *DECONV, f16=True, layouts=(1, 1, 1))),
    "deconv_f16pw_both_classes": ({}, 0, lambda b: run_deconv3d(b, *DECONV, f16=True, layouts=(1, 1, 1))),
    "deconv_f16pw_class_by_class": ({"RT_F16P_CLASSES": "0"}, 0, lambda b: run_deconv3d(b, *DECONV, f16=True, layouts=(1, 1, 1))),
    "deconv_f16pw_segments": ({"RT_F16P_WALK": "2"}, 0, lambda b: run_deconv3d(b, 32, 32, (5, 6, 33), 11, 10, 0, f16=True, layouts=(1, 1, 1))),
    # the tower block, streaming form: kernel by tensor form ...
    "rbs_0": ({}, 0, lambda b: run_block(b, 17, 31, 2)),
    "rbs_1": ({}, 0, lambda b: run_block(b, 17, 31, 2, split=(0, 1))),
    "rbd_0": ({}, 0, lambda b: run_block(b, 17, 31, 2, split=(1, 0))),
    "rbd_1": ({}, 0, lambda b: run_block(b, 17, 31, 2, split=(1, 1))),
    "f16rbd": ({}, 0, lambda b: run_block(b, 17, 31, 2, f16=True, pitch=64)),
    "rbs_seg_knob": ({"RT_RBS_SEG": "9"}, 0, lambda b: run_block(b, 17, 31, 1)),
    # ... and rows per workgroup: 64 under the throughput hint while that leaves 120 workgroups, else 32 while that does, else 16
    "rb_120_hint": ({}, 0, lambda b: run_block(b, 1, 1, 120, hints=HINT)),
    "rb_120": ({}, 0, lambda b: run_block(b, 1, 1, 120)),
    "rb_119_hint": ({}, 0, lambda b: run_block(b, 1, 1, 119, hints=HINT)),
    "rb_119": ({}, 0, lambda b: run_block(b, 1, 1, 119)),
    # ... the per-tile form
    "s3rb_planar": ({}, 1, lambda b: run_block(b, 9, 33, 1, c=16, cmid=24, il=False)),
    "s3rb_interleaved": ({"RT_RB_TILES": "1"}, 1, lambda b: run_block(b, 9, 33, 2)),
    # first layers
    "s3_first": ({}, 0, lambda b: run2d(b, conv2d(b, 3, 32, 9, 35, k=5, stride=2), n=2)),
    "s3_first_interleaved": ({}, 0, lambda b: run2d(b, il(conv2d(b, 3, 32, 9, 35, k=5, stride=2), 0, 1), n=2)),
    "s3_first_twin": ({}, 0, lambda b: run2d(b, il(conv2d(b, 3, 32, 9, 35, k=5, stride=2), 0, 1), twin=True)),
    "s3_first_twin_planar": ({}, 0, lambda b: run2d(b, conv2d(b, 3, 32, 9, 35, k=5, stride=2), n=2, twin=True)),
    "f16_first": ({}, 0, lambda b: run2d(b, io(conv2d(b, 3, 32, 9, 35, k=5, stride=2, pitch=(0, 64)), F32, F16), n=2, y16=True)),
    "f16_first_interleaved": ({}, 0, lambda b: run2d(b, il(io(conv2d(b, 3, 32, 9, 35, k=5, stride=2, pitch=(0, 64)), F32, F16), 0, 1), y16=True)),
    "f16_first_twin": ({}, 0, lambda b: run2d(b, il(io(conv2d(b, 3, 32, 9, 35, k=5, stride=2, pitch=(0, 64)), F32, F16), 0, 1), y16=True, twin=True)),
    # conv_s3: window, layouts, storage types, split-K (a sample's workgroups per CU x chunks of 16 channels; none under the hint)
    "s3_3x3": ({}, 0, lambda b: run2d(b, conv2d(b, 16, 32, 9, 35), n=2)),
    "s3_3x3_interleaved": ({}, 0, lambda b: run2d(b, il(conv2d(b, 32, 32, 9, 35, resid=True), 1, 1, 1), resid=True)),
    "s3_3x3_interleaved_in": ({}, 0, lambda b: run2d(b, il(conv2d(b, 32, 32, 9, 35), 1, 0))),
    "s3_3x3_interleaved_out": ({}, 0, lambda b: run2d(b, il(conv2d(b, 32, 32, 9, 35), 0, 1))),
    "s3_3x3_stride_2": ({}, 0, lambda b: run2d(b, il(conv2d(b, 32, 64, 9, 35, stride=2), 1, 1))),
    "s3_2x2_phases": ({}, 0, lambda b: run2d(b, il(conv2d(b, 64, 32, 5, 33, stride=2, tr=True, resid=True), 1, 1, 1), resid=True)),
    "s3_2x2_phases_planar": ({}, 0, lambda b: run2d(b, conv2d(b, 16, 8, 5, 33, stride=2, tr=True))),
    "s3_ks4": ({}, 0, lambda b: run2d(b, conv2d(b, 64, 32, 9, 35))),
    "s3_ks4_hint": ({}, 0, lambda b: run2d(b, conv2d(b, 64, 32, 9, 35), hints=HINT)),
    "s3_ks2_hint": ({}, 0, lambda b: run2d(b, conv2d(b, 32, 32, 9, 35), hints=HINT)),
    "s3_ksplit_knob": ({"RT_S3_KSPLIT": "2"}, 0, lambda b: run2d(b, conv2d(b, 64, 32, 9, 35), hints=HINT)),
    "s3_no_ksplit_knob": ({"RT_S3_KSPLIT": "0"}, 0, lambda b: run2d(b, conv2d(b, 64, 32, 9, 35))),
    "s3_f16_storage": ({}, 0, lambda b: run_conv3d(b, 8, 32, 5, 9, 35, f16=True)),
    "s3_f16_storage_f32_in": ({}, 0, lambda b: run_conv3d(b, 8, 32, 5, 9, 35, f16=True, x16=False)),
    "s3_f16_storage_stride_2": ({}, 0, lambda b: run_conv3d(b, 16, 24, 5, 8, 37, f16=True, stride=2)),
    "s3_3d": ({}, 0, lambda b: run_conv3d(b, 16, 32, 3, 9, 35, f16=False)),
    "s3_3d_channel_blocks_folded": ({}, 0, lambda b: run_conv3d(b, 16, 64, 3, 9, 35, f16=False)),
    "s3_3d_z_folded": ({"RT_Z_INNER": "2"}, 0, lambda b: run_conv3d(b, 16, 64, 3, 9, 35, f16=False)),
    "s3_3d_nothing_folded": ({"RT_NB_INNER": "0"}, 0, lambda b: run_conv3d(b, 16, 64, 3, 9, 35, f16=False)),
    "s3_8_rows": ({"RT_S3_ROWS": "8"}, 1, lambda b: run2d(b, il(conv2d(b, 32, 32, 9, 35), 1, 1))),
    # Conv3D between interleaved fp16 tensors: the depth walk (resident / streamed weights, skip tensor, activation), what its fill rule
    # declines, four rows per wave, and the 4 x 32 tile below 12 output rows
    "f16dw_resident": (DW, 0, lambda b: run_conv3d(b, 16, 32, 5, 13, 37, f16=True, il=True)),
    "f16dw_resident_skip": (DW, 0, lambda b: run_conv3d(b, 32, 32, 6, 14, 33, f16=True, il=True, resid=True)),
    "f16dw_streamed": (DW, 0, lambda b: run_conv3d(b, 48, 24, 3, 9, 70, f16=True, il=True)),
    "f16dw_streamed_skip_no_act": (DW, 0, lambda b: run_conv3d(b, 64, 32, 5, 13, 40, f16=True, il=True, resid=True, act=NONE)),
    "f16dw_segments": ({"RT_F16_DW": "1", "RT_DW_NSEG": "2"}, 0, lambda b: run_conv3d(b, 32, 64, 4, 12, 40, f16=True, il=True, cm=True)),
    "f16dw_declined": ({}, 0, lambda b: run_conv3d(b, 16, 32, 5, 13, 37, f16=True, il=True)),
    "f16dw_off": ({"RT_F16_DW": "0"}, 0, lambda b: run_conv3d(b, 32, 64, 2, 17, 70, f16=True, il=True, resid=True)),
    "f16mma_below_12_rows": ({}, 0, lambda b: run_conv3d(b, 16, 32, 5, 9, 35, f16=True, il=True)),
    "f16mma_r4_off": ({"RT_F16_R4": "0"}, 0, lambda b: run_conv3d(b, 16, 32, 5, 13, 37, f16=True, il=True)),
    "f16mma_stride_2": ({}, 0, lambda b: run_conv3d(b, 16, 24, 5, 8, 37, f16=True, il=True, stride=2, cm=True)),
    "f16mma_2d": ({}, 0, lambda b: run2d(b, io(conv2d(b, 32, 32, 9, 37, pitch=(64, 64)), F16, F16), x16=True, y16=True)),
    "f16mma_2d_interleaved_r4_knob": ({"RT_F16_R4": "1"}, 0, lambda b: run2d(b, il(io(conv2d(b, 32, 32, 9, 37, pitch=(64, 64)), F16, F16), 1, 1), x16=True, y16=True)),
    # the persistent split kernel
    "s3p": ({"RT_S3P": "1"}, 1, lambda b: run2d(b, il(conv2d(b, 32, 32, 19, 70), 1, 1), n=2)),
    "s3p_grid_knob": ({"RT_S3P": "1", "RT_S3P_GRID": "3"}, 1, lambda b: run2d(b, conv2d(b, 32, 32, 19, 70), n=2)),
    # families without a trace line: nothing is printed, the output is written
    "direct": ({}, 0, lambda b: finite(run2d(b, conv2d(b, 8, 2, 9, 35), n=2))),
    "wino": ({}, 0, lambda b: finite(run2d(b, conv2d(b, 16, 32, 9, 35, flags=EXACT), n=2))),
    "mfma_f32": ({}, 0, lambda b: finite(run2d(b, conv2d(b, 16, 32, 9, 35, stride=2, flags=EXACT), n=2))),
}


def io(plan, x, y):
    plan.set_io_types(x, y)
    return plan


def il(plan, *layouts):
    plan.set_layouts(*layouts)
    return plan


# Recorded on the commit before the enqueue was split into launchers, on the emulator; the same lines on the MI355X.
EXPECTED = {
    'small_2d_f32': ['[rt] deconv3d_s2_small<1,0,f32,f32> grid 1 x 5 x 1'],
    'small_2d_f16': ['[rt] deconv3d_s2_small<1,0,f16,f16> grid 1 x 5 x 1'],
    'small_3d_f32': ['[rt] deconv3d_s2_small<1,1,f32,f32> grid 1 x 4 x 6'],
    'small_3d_f16_in': ['[rt] deconv3d_s2_small<1,1,f16,f32> grid 1 x 4 x 6'],
    'small_3d_two_channels': ['[rt] deconv3d_s2_small<2,1,f32,f32> grid 1 x 3 x 4'],
    'small_il': ['[rt] deconv3d_s2_il grid 3 x 2 x 2'],
    'small_il_64_channels': ['[rt] deconv3d_s2_il grid 2 x 2 x 2'],
    'small_il4': ['[rt] deconv3d_s2_il4 grid 3 x 2 x 2'],
    'small_ilw_one_segment': ['[rt] deconv3d_s2_ilw<0> grid 1 x 2 x 2 segments 1 x 3'],
    'small_ilw_two_segments': ['[rt] deconv3d_s2_ilw<0> grid 2 x 2 x 2 segments 2 x 9'],
    'small_ilw_softargmax': ['[rt] deconv3d_s2_ilw<1> grid 1 x 2 x 2 segments 1 x 3'],
    'small_ilw_softargmin': ['[rt] deconv3d_s2_ilw<2> grid 1 x 2 x 2 segments 1 x 17'],
    'deconv_s3p_planar': ['[rt] deconv_s3p<0> r0 grid 1 x 1 x 6', '[rt] deconv_s3p<0> r0 grid 1 x 1 x 6'],
    'deconv_s3p_interleaved_out': ['[rt] deconv_s3p<1> r1 grid 1 x 1 x 6', '[rt] deconv_s3p<1> r1 grid 1 x 1 x 6'],
    'deconv_f16p': ['[rt] deconv_f16p grid 3 x 1 x 2', '[rt] deconv_f16p grid 3 x 1 x 2'],
    'deconv_f16pw_both_classes': ['[rt] deconv_f16pw grid 3 x 1 x 2, 1 slice indices per segment, 2 class(es)'],
    'deconv_f16pw_class_by_class': ['[rt] deconv_f16pw grid 3 x 1 x 2, 1 slice indices per segment, 1 class(es)',
                                    '[rt] deconv_f16pw grid 3 x 1 x 2, 1 slice indices per segment, 1 class(es)'],
    'deconv_f16pw_segments': ['[rt] deconv_f16pw grid 8 x 1 x 2, 3 slice indices per segment, 2 class(es)'],
    'rbs_0': ['[rt] conv_s3rbs<0> grid 4 x 1 x 2 seg 16'],
    'rbs_1': ['[rt] conv_s3rbs<1> grid 4 x 1 x 2 seg 16'],
    'rbd_0': ['[rt] conv_s3rbd<0> grid 4 x 1 x 2 seg 16'],
    'rbd_1': ['[rt] conv_s3rbd<1> grid 4 x 1 x 2 seg 16'],
    'f16rbd': ['[rt] conv_f16rbd grid 4 x 1 x 2 seg 16'],
    'rbs_seg_knob': ['[rt] conv_s3rbs<0> grid 4 x 1 x 1 seg 12'],
    'rb_120_hint': ['[rt] conv_s3rbs<0> grid 1 x 1 x 120 seg 64'],
    'rb_120': ['[rt] conv_s3rbs<0> grid 1 x 1 x 120 seg 32'],
    'rb_119_hint': ['[rt] conv_s3rbs<0> grid 1 x 1 x 119 seg 16'],
    'rb_119': ['[rt] conv_s3rbs<0> grid 1 x 1 x 119 seg 16'],
    's3rb_planar': ['[rt] conv_s3rb x0 y0 grid 6 x 1'],
    's3rb_interleaved': ['[rt] conv_s3rb x1 y1 grid 6 x 2'],
    's3_first': ['[rt] conv_s3_first<0> grid 2 x 1 x 2 twin 0'],
    's3_first_interleaved': ['[rt] conv_s3_first<1> grid 2 x 1 x 2 twin 0'],
    's3_first_twin': ['[rt] conv_s3_first<1> grid 2 x 1 x 2 twin 1'],
    's3_first_twin_planar': ['[rt] conv_s3_first<0> grid 2 x 1 x 4 twin 1'],
    'f16_first': ['[rt] conv_f16_first<0> grid 2 x 1 x 2 twin 0'],
    'f16_first_interleaved': ['[rt] conv_f16_first<1> grid 2 x 1 x 1 twin 0'],
    'f16_first_twin': ['[rt] conv_f16_first<1> grid 2 x 1 x 2 twin 1'],
    's3_3x3': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 6 x 1 x 2 ks 1'],
    's3_3x3_interleaved': ['[rt] conv_s3<3,3,1,1,1,4,f32,f32> r1 grid 6 x 1 x 1 ks 2'],
    's3_3x3_interleaved_in': ['[rt] conv_s3<3,3,1,1,0,4,f32,f32> r0 grid 6 x 1 x 1 ks 2'],
    's3_3x3_interleaved_out': ['[rt] conv_s3<3,3,1,0,1,4,f32,f32> r0 grid 6 x 1 x 1 ks 2'],
    's3_3x3_stride_2': ['[rt] conv_s3<3,3,2,1,1,4,f32,f32> r0 grid 2 x 2 x 1 ks 2'],
    's3_2x2_phases': ['[rt] conv_s3<2,2,1,1,1,4,f32,f32> r1 grid 4 x 1 x 4 ks 4'],
    's3_2x2_phases_planar': ['[rt] conv_s3<2,2,1,0,0,4,f32,f32> r0 grid 4 x 1 x 4 ks 1'],
    's3_ks4': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 6 x 1 x 1 ks 4'],
    's3_ks4_hint': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 6 x 1 x 1 ks 1'],
    's3_ks2_hint': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 6 x 1 x 1 ks 1'],
    's3_ksplit_knob': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 6 x 1 x 1 ks 2'],
    's3_no_ksplit_knob': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 6 x 1 x 1 ks 1'],
    's3_f16_storage': ['[rt] conv_s3<3,3,1,0,0,4,f16,f16> r0 grid 6 x 1 x 10 ks 2'],
    's3_f16_storage_f32_in': ['[rt] conv_s3<3,3,1,0,0,4,f32,f16> r0 grid 6 x 1 x 10 ks 2'],
    's3_f16_storage_stride_2': ['[rt] conv_s3<3,3,2,0,0,4,f16,f16> r0 grid 1 x 1 x 6 ks 2'],
    's3_3d': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 6 x 1 x 6 ks 2'],
    's3_3d_channel_blocks_folded': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 12 x 1 x 6 ks 2'],
    's3_3d_z_folded': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 36 x 1 x 2 ks 2'],
    's3_3d_nothing_folded': ['[rt] conv_s3<3,3,1,0,0,4,f32,f32> r0 grid 6 x 2 x 6 ks 2'],
    's3_8_rows': ['[rt] conv_s3<3,3,1,1,1,8,f32,f32> r0 grid 4 x 1 x 1 ks 1'],
    'f16dw_resident': ['[rt] conv_f16dw<1,0,1> grid 2 x 2 segments 1 x 5 slices, 1 chunks per slice'],
    'f16dw_resident_skip': ['[rt] conv_f16dw<1,1,1> grid 2 x 2 segments 1 x 6 slices, 2 chunks per slice'],
    'f16dw_streamed': ['[rt] conv_f16dw<0,0,1> grid 2 x 2 segments 1 x 3 slices, 3 chunks per slice'],
    'f16dw_streamed_skip_no_act': ['[rt] conv_f16dw<0,1,0> grid 2 x 2 segments 1 x 5 slices, 4 chunks per slice'],
    'f16dw_segments': ['[rt] conv_f16dw<1,0,1> grid 4 x 2 segments 2 x 2 slices, 2 chunks per slice'],
    'f16dw_declined': ['[rt] conv_f16r4 grid 10 x 1 x 2'],
    'f16dw_off': ['[rt] conv_f16r4 grid 24 x 1 x 2'],
    'f16mma_below_12_rows': ['[rt] conv_f16mma 3x3 s1 rows 4 il8 x1 y1 r0 grid 6 x 1 x 10'],
    'f16mma_r4_off': ['[rt] conv_f16mma 3x3 s1 rows 4 il8 x1 y1 r0 grid 8 x 1 x 10'],
    'f16mma_stride_2': ['[rt] conv_f16mma 3x3 s2 rows 4 il8 x1 y1 r0 grid 1 x 1 x 6'],
    'f16mma_2d': ['[rt] conv_f16mma 3x3 s1 rows 4 il8 x0 y0 r0 grid 6 x 1 x 1'],
    'f16mma_2d_interleaved_r4_knob': ['[rt] conv_f16r4 grid 2 x 1 x 1'],
    's3p': ['[rt] conv_s3p x1 y1 r0 tiles 18 grid 16'],
    's3p_grid_knob': ['[rt] conv_s3p x0 y0 r0 tiles 18 grid 3'],
    'direct': [],
    'wino': [],
    'mfma_f32': [],
}


@pytest.mark.parametrize("name", list(CASES))
def test_conv_dispatch(backend, monkeypatch, capfd, name):
    env, experimental, run = CASES[name]
    if experimental and not backend.klib.has_experimental():
        pytest.skip("a rejected kernel family, compiled with RT_EXPERIMENTAL only (the emulator build of the CPU tier)")
    monkeypatch.setenv("RT_CONV_TRACE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    run(backend)
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[rt] ")]
    print(name, lines)
    assert lines == EXPECTED[name]
