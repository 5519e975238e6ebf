"""Stored forms of the activation tensors the kernels read and write, shared by the parity tests: pitched rows, channel-interleaved groups,
pre-split (hi | lo) fp16 records."""
import numpy as np


def pitched(a, pitch, fill=np.nan):
    """(..., H, W) -> (..., H, pitch) with `fill` in the padding columns"""
    out = np.full(a.shape[:-1] + (pitch,), fill, np.float32)
    out[..., :a.shape[-1]] = a
    return out


def to_il(a, g):
    """(N, C, H, P) planar -> (N, C/g, H, P, g) channel-interleaved"""
    n, c, h, p = a.shape
    return np.ascontiguousarray(a.reshape(n, c // g, g, h, p).transpose(0, 1, 3, 4, 2))


def from_il(a):
    n, q, h, p, g = a.shape
    return a.transpose(0, 1, 4, 2, 3).reshape(n, q * g, h, p)


def to_split(a):
    """(N, C, H, P) fp32 -> the pre-split tensor (N, C/8, H, P, [8 hi | 8 lo]) as an fp32-typed array (N, C/8, H, P, 8):
    hi = fp16(v), lo = fp16((v - hi) * 2^11) (include/rt_stereo.h: rt_resblock_plan_set_split)"""
    n, c, h, p = a.shape
    g = a.reshape(n, c // 8, 8, h, p).transpose(0, 1, 3, 4, 2).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        hi = g.astype(np.float16)
        lo = ((g - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return np.ascontiguousarray(np.concatenate([hi, lo], axis=-1)).view(np.float32)


def from_split(a):
    """the values a pre-split tensor holds, hi + lo * 2^-11, as (N, C, H, P) fp32"""
    h16 = np.ascontiguousarray(a).view(np.float16)
    n, g, h, p, _ = h16.shape
    v = h16[..., :8].astype(np.float32) + h16[..., 8:].astype(np.float32) * np.float32(1 / 2048)
    return v.transpose(0, 1, 4, 2, 3).reshape(n, g * 8, h, p)
