"""ctypes binding of the C ABI in include/rt_stereo.h (+ the net-level ABI in include/rt_stereo_net.h).

This is plumbing for tests and bench.py: PyTorch (or numpy under the test-only emulator) owns the
buffers, the C ABI does the work.  There is no Python/torch compute fallback: if the HIP library is
missing, or no GPU is visible, loading fails loudly.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# RT_LIB_DIR: another build of the two libraries (redtail_amd/build.py: build_variant) for A/B measurements with bench.py / tools
_LIB_DIR = os.environ.get("RT_LIB_DIR") or os.path.join(ROOT, "redtail_amd", "lib")
HIP_LIB = os.path.join(_LIB_DIR, "librt_stereo_hip.so")
HOST_LIB = os.path.join(_LIB_DIR, "libnvstereo_inference.so")

RT_F32, RT_F16 = 0, 1
RT_NCHW, RT_NC2HW2 = 0, 1
RT_ACT_NONE, RT_ACT_ELU, RT_ACT_SIGMOID = 0, 1, 2


RT_ENC_BGR8, RT_ENC_RGB8, RT_ENC_BGRA8, RT_ENC_RGBA8 = 0, 1, 2, 3     # sensor_msgs/Image encodings (rt_preprocess_frames_u8)
ENC_BYTES = {RT_ENC_BGR8: 3, RT_ENC_RGB8: 3, RT_ENC_BGRA8: 4, RT_ENC_RGBA8: 4}
# wire encodings of sensor_msgs/Image that only rt_decode_frames_u8 / rtDecodeCall take: mono, Bayer (the letters are the top-left 2 x 2, row-major), YUV 4:2:2
RT_WIRE_MONO8, RT_WIRE_MONO16 = 16, 17
RT_WIRE_BAYER_RGGB8, RT_WIRE_BAYER_BGGR8, RT_WIRE_BAYER_GBRG8, RT_WIRE_BAYER_GRBG8 = 18, 19, 20, 21
RT_WIRE_YUV422, RT_WIRE_YUV422_YUY2 = 22, 23                          # UYVY, YUYV
WIRE_BYTES = {RT_WIRE_MONO8: 1, RT_WIRE_MONO16: 2, RT_WIRE_BAYER_RGGB8: 1, RT_WIRE_BAYER_BGGR8: 1, RT_WIRE_BAYER_GBRG8: 1, RT_WIRE_BAYER_GRBG8: 1,
              RT_WIRE_YUV422: 2, RT_WIRE_YUV422_YUY2: 2}
RT_DISP_NET, RT_DISP_PIXELS_F32, RT_DISP_KITTI_U16 = 0, 1, 2          # forms of a disparity output (rt_lr_consistency, rt_net_execute_frames)
RT_DEPTH_M_F32, RT_DEPTH_MM_U16 = 0, 1                                # REP 118 depth images (rt_disparity_to_points)
RT_HINT_THROUGHPUT = 1     # include/rt_stereo.h
RT_CONV_EXACT_FP32 = 1     # rtConv2dDesc.flags / rtConv3dDesc.flags / rtNetOptions.flags


class RtError(RuntimeError):
    pass


class Conv2dDesc(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("Cin", "Cout", "Hin", "Win", "KH", "KW", "stride", "pad_h", "pad_w", "act",
                                     "has_residual", "dtype", "flags")]


class StereoCamera(ctypes.Structure):
    """rtStereoCamera (include/rt_stereo.h): a rectified pair in the geometry of the output; from sensor_msgs/CameraInfo fx = P[0], fy = P[5],
    cx = P[2], cy = P[6] of the left camera, baseline = -P_right[3] / P_right[0] (metres), doffs = P_right[2] - P_left[2] (pixels)"""
    _fields_ = [(n, c_float) for n in ("fx", "fy", "cx", "cy", "baseline", "doffs")]


class RectifyCamera(ctypes.Structure):
    """rtRectifyCamera (include/rt_stereo.h): one camera of a raw rig.  d: k1 k2 p1 p2 k3 k4 k5 k6; iR: inverse of P[:, :3] * R"""
    _fields_ = [("fx", c_double), ("fy", c_double), ("cx", c_double), ("cy", c_double), ("d", c_double * 8), ("iR", c_double * 9)]

    @classmethod
    def from_camera_info(cls, K, D, R, P, lib=None):
        """from the fields of a sensor_msgs/CameraInfo (K, R: 9 values, P: 12, D: 0, 4, 5 or 8) through rt_rectify_camera_from_info of
        `lib` (a KernelLib; default: the product library)"""
        import numpy as np
        k, r, pm = (np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1)) for a in (K, R, P))
        dd = np.ascontiguousarray(np.asarray(D if D is not None else [], np.float64).reshape(-1))
        if k.size != 9 or r.size != 9 or pm.size != 12:
            raise ValueError("K and R hold 9 values, P holds 12")
        lib = lib if lib is not None else KernelLib()
        cam = cls()
        as_p = lambda a: a.ctypes.data_as(POINTER(c_double))
        lib.check(lib.lib.rt_rectify_camera_from_info(as_p(k), as_p(dd) if dd.size else None, int(dd.size), as_p(r), as_p(pm), ctypes.byref(cam)),
                  "rt_rectify_camera_from_info")
        return cam


class VoxelGrid(ctypes.Structure):
    """rtVoxelGrid (include/rt_stereo.h): origin, leaf and dims per axis x, y, z; camera frame, metres"""
    _fields_ = [("origin", c_float * 3), ("leaf", c_float * 3), ("dims", c_int * 3)]

    @classmethod
    def make(cls, origin, leaf, dims):
        leaf = (leaf,) * 3 if isinstance(leaf, (int, float)) else leaf
        return cls((c_float * 3)(*origin), (c_float * 3)(*leaf), (c_int * 3)(*dims))


class Conv3dDesc(ctypes.Structure):
    _fields_ = [("C", c_int), ("K", c_int), ("D", c_int), ("H", c_int), ("W", c_int), ("kernel", c_int * 3),
                ("stride", c_int * 3), ("pad_start", c_int * 3), ("pad_end", c_int * 3), ("act", c_int),
                ("out_dchw", c_int), ("has_residual", c_int), ("dtype", c_int), ("out_depth", c_int),
                ("in_pad_end", c_int), ("cv_fold", c_int), ("flags", c_int)]


# name -> (restype, argtypes); every symbol declared in include/rt_stereo.h
KERNEL_SYMBOLS = {
    "rt_last_error_string": (c_char_p, []),
    "rt_backend_name": (c_char_p, []),
    "rt_device_count": (c_int, []),
    "rt_set_device": (c_int, [c_int]),
    "rt_malloc": (c_int, [POINTER(c_void_p), c_size_t]),
    "rt_free": (c_int, [c_void_p]),
    "rt_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "rt_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "rt_memcpy_d2d": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "rt_memset": (c_int, [c_void_p, c_int, c_size_t, c_void_p]),
    "rt_stream_create": (c_int, [POINTER(c_void_p)]),
    "rt_stream_destroy": (c_int, [c_void_p]),
    "rt_stream_sync": (c_int, [c_void_p]),
    "rt_stream_wait_event": (c_int, [c_void_p, c_void_p]),
    "rt_event_create": (c_int, [POINTER(c_void_p)]),
    "rt_event_create_ordering": (c_int, [POINTER(c_void_p)]),
    "rt_event_destroy": (c_int, [c_void_p]),
    "rt_event_record": (c_int, [c_void_p, c_void_p]),
    "rt_event_elapsed_ms": (c_int, [c_void_p, c_void_p, POINTER(c_float)]),
    "rt_elu": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "rt_add_act": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "rt_activation": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "rt_corr_cost_volume": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 7 + [c_void_p]),
    "rt_corr_cost_volume_flags": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 7 + [ctypes.c_uint, c_void_p]),
    "rt_cost_volume": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    "rt_softargmax": (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    "rt_corr_softargmax": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_int64, c_int, c_void_p]),
    "rt_corr_softargmax_flags": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_int64, c_int, ctypes.c_uint, c_void_p]),
    "rt_corr_softargmax_pitched": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 8 + [c_int64, c_int, c_void_p]),
    "rt_corr_softargmax_il": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 8 + [c_int64, c_void_p]),
    "rt_corr_softargmax_il_slot": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 8 + [c_int64, c_int, c_void_p]),
    "rt_corr_softargmax_il8_f16": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 8 + [c_int64, c_int, c_void_p]),
    "rt_permute4d": (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [POINTER(c_int), c_int, c_void_p]),
    "rt_convert_format": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_int, c_void_p]),
    "rt_pad_d": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_int, c_void_p]),
    "rt_slice_d": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_int, c_int, c_void_p]),
    "rt_concat_channels": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_int, c_void_p]),
    "rt_conv2d_plan_create": (c_int, [POINTER(c_void_p), POINTER(Conv2dDesc), c_void_p, c_void_p]),
    "rt_deconv2d_plan_create": (c_int, [POINTER(c_void_p), POINTER(Conv2dDesc), c_void_p, c_void_p]),
    "rt_resblock_plan_create": (c_int, [POINTER(c_void_p), POINTER(Conv2dDesc), c_void_p, c_void_p, POINTER(Conv2dDesc), c_void_p,
                                        c_void_p]),
    "rt_conv3d_plan_create": (c_int, [POINTER(c_void_p), POINTER(Conv3dDesc), c_void_p, c_void_p]),
    "rt_conv3d_transpose_plan_create": (c_int, [POINTER(c_void_p), POINTER(Conv3dDesc), POINTER(c_int), c_void_p,
                                                c_void_p]),
    "rt_preprocess_bgr8": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "rt_disparity_to_u16": (c_int, [c_void_p, c_void_p, c_int64, ctypes.c_float, c_void_p]),
    "rt_preprocess_frames_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                        c_void_p]),
    "rt_disparity_scale": (c_int, [c_void_p, c_void_p, c_int64, ctypes.c_float, c_void_p]),
    "rt_preprocess_frames_u8_lr": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                           c_void_p]),
    "rt_lr_consistency": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_preprocess_frames_u8_cv": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                           c_void_p]),
    "rt_disparity_to_frame": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "rt_points_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rt_disparity_to_points": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(StereoCamera), c_float, c_float, c_void_p,
                                       c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_size_t, c_void_p]),
    "rt_speckle_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rt_voxel_workspace_bytes": (c_size_t, [c_int, c_int, c_void_p]),
    "rt_points_voxel_grid": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_size_t, c_void_p]),
    "rt_disparity_speckle": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    "rt_rectify_camera_from_info": (c_int, [POINTER(c_double), POINTER(c_double), c_int, POINTER(c_double), POINTER(c_double),
                                            POINTER(RectifyCamera)]),
    "rt_rectify_frames_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, POINTER(RectifyCamera), POINTER(RectifyCamera), c_void_p,
                                     c_void_p, c_int, c_int, c_int64, c_int, c_void_p]),
    "rt_rectify_maps": (c_int, [POINTER(RectifyCamera), c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "rt_remap_frames_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int, c_int, c_int64, c_int, c_void_p]),
    "rt_decode_frames_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "rt_disparity_to_color": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_int64, c_void_p]),
    "rt_viz_mosaic_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_int, c_int, c_float, c_void_p, c_int64, c_int,
                                 c_void_p]),
    "rt_conv_plan_input_limit": (c_int, [c_void_p, POINTER(c_float)]),
    "rt_has_experimental": (c_int, []),
    "rt_graph_begin_capture": (c_int, [c_void_p]),
    "rt_graph_end_capture": (c_int, [c_void_p, POINTER(c_void_p)]),
    "rt_graph_launch": (c_int, [c_void_p, c_void_p]),
    "rt_graph_destroy": (c_int, [c_void_p]),
    "rt_check_range": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_float, POINTER(c_float), POINTER(c_int64), c_void_p]),
    "rt_hash_buffer": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    "rt_conv_plan_out_dims": (c_int, [c_void_p, POINTER(c_int)]),
    "rt_conv_plan_set_pitch": (c_int, [c_void_p, c_int, c_int]),
    "rt_conv_plan_set_batch_strides": (c_int, [c_void_p, c_int64, c_int64, c_int64]),
    "rt_conv_plan_set_io_types": (c_int, [c_void_p, c_int, c_int]),
    "rt_conv_plan_supports_il8": (c_int, [c_void_p]),
    "rt_conv_plan_set_layouts": (c_int, [c_void_p, c_int, c_int, c_int]),
    "rt_conv_plan_set_softarg": (c_int, [c_void_p, c_int]),
    "rt_conv_plan_supports_twin_input": (c_int, [c_void_p]),
    "rt_conv_enqueue_twin_input": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int]),
    "rt_resblock_plan_supports_split": (c_int, [c_void_p]),
    "rt_resblock_plan_set_split": (c_int, [c_void_p, c_int, c_int]),
    "rt_conv_enqueue": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "rt_conv_enqueue_hint": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int]),
    "rt_conv_plan_workspace_bytes": (ctypes.c_size_t, [c_void_p, c_int]),
    "rt_conv_enqueue_ws": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p, c_int]),
    "rt_conv_plan_destroy": (c_int, [c_void_p]),
    # multi-GPU: RCCL communicator + byte broadcast (librccl is loaded on first use)
    "rt_comm_unique_id": (c_int, [c_void_p]),
    "rt_comm_init_rank": (c_int, [POINTER(c_void_p), c_int, c_int, c_void_p]),
    "rt_comm_init_all": (c_int, [POINTER(c_void_p), c_int, POINTER(c_int)]),
    "rt_comm_adopt": (c_int, [POINTER(c_void_p), c_void_p]),
    "rt_comm_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "rt_comm_broadcast": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "rt_comm_group_start": (c_int, []),
    "rt_comm_group_end": (c_int, []),
    "rt_comm_destroy": (c_int, [c_void_p]),
}
RT_COMM_ID_BYTES = 128


def _ptr(x):
    """Raw device address of a torch tensor / numpy array (emulator) / int."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        return x.ctypes.data
    raise TypeError("cannot take the address of %r" % type(x))


def _host_weights(a, dtype, what):
    """Plan constructors read host weight / bias arrays through a raw pointer: refuse an array of another element type (a float32
    array divided by np.sqrt(...) is float64 under NumPy 2 and would be read as garbage)."""
    if a is not None and hasattr(a, "dtype") and hasattr(a, "ctypes"):
        want = "float16" if dtype == RT_F16 else "float32"
        if a.dtype.name != want:
            raise TypeError("%s: expected a %s array, got %s" % (what, want, a.dtype))
        if not a.flags["C_CONTIGUOUS"]:
            raise TypeError("%s: array is not C-contiguous" % what)
    return a


class KernelLib:
    """The op-level C ABI.  `path=None` loads the gfx950 build and requires a visible GPU."""

    def __init__(self, path=None):
        emulated = path is not None
        path = path or HIP_LIB
        if not os.path.exists(path):
            raise RtError("native library %s is missing -- run `python -m redtail_amd.build` "
                          "(there is no Python fallback for the HIP path)" % path)
        self.path = path
        self.lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in KERNEL_SYMBOLS.items():
            fn = getattr(self.lib, name)      # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        if not emulated and self.lib.rt_device_count() < 1:
            raise RtError("no HIP device visible: the Stereo DNN path runs on MI355X only")

    # -- helpers ---------------------------------------------------------------------------------
    def check(self, rc, what=""):
        if rc != 0:
            raise RtError("%s failed (%d): %s" % (what, rc, self.lib.rt_last_error_string().decode()))

    def backend(self):
        return self.lib.rt_backend_name().decode()

    # -- ops (x/y are torch CUDA tensors, or numpy arrays under the emulator) -----------------------
    def elu(self, x, y, n, dtype=RT_F32, stream=None):
        self.check(self.lib.rt_elu(_ptr(x), _ptr(y), n, dtype, stream), "rt_elu")

    def add_act(self, a, b, y, n, act, dtype=RT_F32, stream=None):
        self.check(self.lib.rt_add_act(_ptr(a), _ptr(b), _ptr(y), n, act, dtype, stream), "rt_add_act")

    def activation(self, x, y, n, act, dtype=RT_F32, stream=None):
        self.check(self.lib.rt_activation(_ptr(x), _ptr(y), n, act, dtype, stream), "rt_activation")

    def corr_cost_volume(self, l, r, cv, batch, C, H, W, D, dtype=RT_F32, fmt=RT_NCHW, stream=None, flags=0):
        self.check(self.lib.rt_corr_cost_volume_flags(_ptr(l), _ptr(r), _ptr(cv), batch, C, H, W, D, dtype, fmt, flags, stream)
                   if flags else self.lib.rt_corr_cost_volume(_ptr(l), _ptr(r), _ptr(cv), batch, C, H, W, D, dtype, fmt, stream),
                   "rt_corr_cost_volume")

    def preprocess_bgr8(self, src, src_h, src_w, dst, dst_h, dst_w, batch=1, stream=None):
        self.check(self.lib.rt_preprocess_bgr8(_ptr(src), src_h, src_w, _ptr(dst), dst_h, dst_w, batch, stream),
                   "rt_preprocess_bgr8")

    def disparity_to_u16(self, disp, out, n, scale, stream=None):
        self.check(self.lib.rt_disparity_to_u16(_ptr(disp), _ptr(out), n, scale, stream), "rt_disparity_to_u16")

    def preprocess_frames_u8(self, left, right, src_h, src_w, src_step, encoding, left_dst, right_dst, dst_h, dst_w, batch=1,
                             stream=None):
        """both frames of a pair batch, rows src_step bytes apart, RT_ENC_* encoding -> two (N,3,dst_h,dst_w) fp32 RGB batches"""
        self.check(self.lib.rt_preprocess_frames_u8(_ptr(left), _ptr(right), src_h, src_w, src_step, encoding, _ptr(left_dst),
                                                    _ptr(right_dst), dst_h, dst_w, batch, stream), "rt_preprocess_frames_u8")

    def disparity_scale(self, disp, out, n, scale, stream=None):
        self.check(self.lib.rt_disparity_scale(_ptr(disp), _ptr(out), n, scale, stream), "rt_disparity_scale")

    def preprocess_frames_u8_lr(self, left, right, src_h, src_w, src_step, encoding, left_dst, right_dst, dst_h, dst_w, batch=1,
                                stream=None):
        """preprocess_frames_u8 into images [0, batch) of two (2N,3,dst_h,dst_w) batches, plus the mirrored, swapped pair as [batch, 2N)"""
        self.check(self.lib.rt_preprocess_frames_u8_lr(_ptr(left), _ptr(right), src_h, src_w, src_step, encoding, _ptr(left_dst),
                                                       _ptr(right_dst), dst_h, dst_w, batch, stream), "rt_preprocess_frames_u8_lr")

    def lr_consistency(self, net_disp, batch, h, w, scale, max_diff_px, out, kind=1, mask=None, right_out=None, valid_count=None,
                       stream=None):
        """left-right check of a (2N,1,h,w) engine output of the batch above: (N,1,h,w) `out` in `kind` (RT_DISP_*: 0 raw, 1 pixels,
        2 KITTI uint16) with inconsistent pixels 0, uint8 mask (255 = consistent), right view's disparity, uint64 count per image"""
        self.check(self.lib.rt_lr_consistency(_ptr(net_disp), batch, h, w, scale, max_diff_px, _ptr(out), kind, _ptr(mask),
                                              _ptr(right_out), _ptr(valid_count), stream), "rt_lr_consistency")

    def preprocess_frames_u8_cv(self, left, right, src_h, src_w, src_step, encoding, left_dst, right_dst, dst_h, dst_w, batch=1,
                                mirror_twin=False, stream=None):
        """preprocess_frames_u8 for any size: cv::resize(INTER_AREA) as a whole (box filter when neither axis grows, else two taps an axis);
        mirror_twin: the destinations hold 2N images, [batch, 2N) the mirrored, swapped pair of preprocess_frames_u8_lr"""
        self.check(self.lib.rt_preprocess_frames_u8_cv(_ptr(left), _ptr(right), src_h, src_w, src_step, encoding, _ptr(left_dst),
                                                       _ptr(right_dst), dst_h, dst_w, batch, int(bool(mirror_twin)), stream),
                   "rt_preprocess_frames_u8_cv")

    def disparity_to_frame(self, disp_px, batch, h, w, out, out_h, out_w, kind=1, mask=None, out_mask=None, valid_count=None, stream=None):
        """(N,1,h,w) fp32 disparity in the network's pixels (+ the uint8 mask of lr_consistency) -> (N,1,out_h,out_w) in the frame's
        pixels, `kind` RT_DISP_PIXELS_F32 or RT_DISP_KITTI_U16; with a mask: the frame's uint8 mask and uint64 count per image"""
        self.check(self.lib.rt_disparity_to_frame(_ptr(disp_px), _ptr(mask), batch, h, w, _ptr(out), kind, out_h, out_w, _ptr(out_mask),
                                                  _ptr(valid_count), stream), "rt_disparity_to_frame")

    def rectify_frames_u8(self, left, right, src_h, src_w, src_step, encoding, cam_left, cam_right, left_dst, right_dst, dst_h, dst_w,
                          dst_step, batch=1, stream=None):
        """raw frames -> rectified frames of the same encoding, both frames of a pair batch in one launch: initUndistortRectifyMap's model
        per pixel in double, remap(INTER_LINEAR, BORDER_CONSTANT 0) in fp32.  cam_left / cam_right: RectifyCamera"""
        self.check(self.lib.rt_rectify_frames_u8(_ptr(left), _ptr(right), src_h, src_w, src_step, encoding,
                                                 ctypes.byref(cam_left) if cam_left is not None else None,
                                                 ctypes.byref(cam_right) if cam_right is not None else None, _ptr(left_dst), _ptr(right_dst),
                                                 dst_h, dst_w, dst_step, batch, stream), "rt_rectify_frames_u8")

    def rectify_maps(self, cam, dst_h, dst_w, map_x, map_y, stream=None):
        """the (dst_h, dst_w) fp32 map pair of one RectifyCamera, as rectify_frames_u8 forms it in registers"""
        self.check(self.lib.rt_rectify_maps(ctypes.byref(cam) if cam is not None else None, dst_h, dst_w, _ptr(map_x), _ptr(map_y), stream),
                   "rt_rectify_maps")

    def remap_frames_u8(self, left, right, src_h, src_w, src_step, encoding, map_x_left, map_y_left, map_x_right, map_y_right, left_dst,
                        right_dst, dst_h, dst_w, dst_step, batch=1, stream=None):
        """rectify_frames_u8's sampler on the caller's own maps (shared by the batch)"""
        self.check(self.lib.rt_remap_frames_u8(_ptr(left), _ptr(right), src_h, src_w, src_step, encoding, _ptr(map_x_left), _ptr(map_y_left),
                                               _ptr(map_x_right), _ptr(map_y_right), _ptr(left_dst), _ptr(right_dst), dst_h, dst_w, dst_step,
                                               batch, stream), "rt_remap_frames_u8")

    def decode_frames_u8(self, left_wire, right_wire, h, w, wire_step, wire_encoding, left_dst, right_dst, dst_step, dst_encoding=RT_ENC_BGR8,
                         batch=1, stream=None):
        """wire frames (RT_WIRE_*: mono8 / mono16, 8-bit Bayer, YUV 4:2:2), rows wire_step bytes apart -> h x w colour frames in dst_encoding
        (RT_ENC_*), rows dst_step bytes apart, both frames of a pair batch in one launch: grey replication, bilinear demosaicing, BT.601"""
        self.check(self.lib.rt_decode_frames_u8(_ptr(left_wire), _ptr(right_wire), h, w, wire_step, wire_encoding, _ptr(left_dst), _ptr(right_dst),
                                                dst_step, dst_encoding, batch, stream), "rt_decode_frames_u8")

    def points_workspace_bytes(self, batch, out_h, out_w):
        """bytes of device workspace disparity_to_points needs for a compact cloud or a count"""
        return self.lib.rt_points_workspace_bytes(batch, out_h, out_w)

    def disparity_to_points(self, disp_px, batch, h, w, out_h, out_w, camera, min_depth=0.0, max_depth=float("inf"), mask=None, color=None,
                            color_step=None, encoding=RT_ENC_BGR8, disp_out=None, disp_kind=RT_DISP_PIXELS_F32, out_mask=None, valid_count=None,
                            depth=None, depth_kind=RT_DEPTH_M_F32, points=None, points_compact=None, count=None, workspace=None,
                            workspace_bytes=None, stream=None):
        """disparity_to_frame plus the reprojection in one launch: (N,1,h,w) fp32 disparity in the network's pixels (+ mask) -> any of the
        frame-geometry disparity (+ mask, count), a REP 118 depth image (RT_DEPTH_M_F32 / RT_DEPTH_MM_U16), the organised cloud
        (N,out_h,out_w) x 16 bytes {x, y, z, rgb}, and -- one more launch, `workspace` of points_workspace_bytes -- the compact cloud with its
        uint64 count per image.  camera: StereoCamera in the output's geometry; color: the left frames (N,out_h,color_step) uint8."""
        if color_step is None:
            color_step = out_w * ENC_BYTES.get(encoding, 0)
        if workspace_bytes is None:
            workspace_bytes = 0 if workspace is None else (workspace.numel() * workspace.element_size() if hasattr(workspace, "numel") else workspace.nbytes)
        self.check(self.lib.rt_disparity_to_points(_ptr(disp_px), _ptr(mask), batch, h, w, out_h, out_w,
                                                   ctypes.byref(camera) if camera is not None else None, min_depth, max_depth, _ptr(color),
                                                   color_step, encoding, _ptr(disp_out), disp_kind, _ptr(out_mask), _ptr(valid_count), _ptr(depth),
                                                   depth_kind, _ptr(points), _ptr(points_compact), _ptr(count), _ptr(workspace), workspace_bytes,
                                                   stream), "rt_disparity_to_points")

    def speckle_workspace_bytes(self, batch, h, w):
        """bytes of device workspace disparity_speckle needs (0 for sizes it refuses)"""
        return self.lib.rt_speckle_workspace_bytes(batch, h, w)

    def disparity_speckle(self, disp_px, batch, h, w, max_size, max_diff_px, out, mask=None, out_mask=None, valid_count=None, workspace=None,
                          workspace_bytes=None, stream=None):
        """the speckle filter (stereo_image_proc's speckle_size / speckle_range, cv::filterSpeckles) on a (N,1,h,w) fp32 disparity (+ the
        255 / 0 mask of lr_consistency): 4-connected components of live pixels whose neighbours differ by <= max_diff_px; those of at most
        max_size pixels become 0 in out and in out_mask.  In place (out = disp_px, out_mask = mask) is legal.  valid_count: N uint64 on the
        device; workspace: speckle_workspace_bytes of device memory."""
        if workspace_bytes is None:
            workspace_bytes = 0 if workspace is None else (workspace.numel() * workspace.element_size() if hasattr(workspace, "numel") else workspace.nbytes)
        self.check(self.lib.rt_disparity_speckle(_ptr(disp_px), _ptr(mask), batch, h, w, max_size, max_diff_px, _ptr(out), _ptr(out_mask),
                                                 _ptr(valid_count), _ptr(workspace), workspace_bytes, stream), "rt_disparity_speckle")

    def voxel_workspace_bytes(self, batch, capacity, grid):
        """bytes of device workspace points_voxel_grid needs (0 for a batch, a capacity or a grid it refuses)"""
        return self.lib.rt_voxel_workspace_bytes(batch, capacity, ctypes.byref(grid) if grid is not None else None)

    def points_voxel_grid(self, points, batch, capacity, grid, voxels, out_capacity, out_count, count=None, min_points=1, out_cell=None,
                          out_n=None, workspace=None, workspace_bytes=None, stream=None):
        """pcl::VoxelGrid on the device: (N, capacity) x 16-byte records {x, y, z, rgb} -- the organised cloud (count=None, NaNs drop out) or
        the compact cloud with its N uint64 `count` -- onto `grid` (VoxelGrid).  voxels: (N, out_capacity) x 16 bytes, the centroid and mean
        colour of every cell with >= min_points points in ascending cell index; out_count: N uint64, the number emitted (> out_capacity:
        truncated); out_cell / out_n: (N, out_capacity) uint32, cell index and point count per record.  workspace: voxel_workspace_bytes of
        device memory.  The result does not depend on the order of the records."""
        if workspace_bytes is None:
            workspace_bytes = 0 if workspace is None else (workspace.numel() * workspace.element_size() if hasattr(workspace, "numel") else workspace.nbytes)
        self.check(self.lib.rt_points_voxel_grid(_ptr(points), _ptr(count), batch, capacity, ctypes.byref(grid) if grid is not None else None,
                                                 min_points, _ptr(voxels), out_capacity, _ptr(out_count), _ptr(out_cell), _ptr(out_n),
                                                 _ptr(workspace), workspace_bytes, stream), "rt_points_voxel_grid")

    def corr_softargmax_pitched(self, l, r, out, batch, C, H, W, D, is_min, in_pitch, out_pitch, out_bstride=0,
                                dtype=RT_F32, stream=None):
        self.check(self.lib.rt_corr_softargmax_pitched(_ptr(l), _ptr(r), _ptr(out), batch, C, H, W, D, int(is_min),
                                                       in_pitch, out_pitch, out_bstride, dtype, stream),
                   "rt_corr_softargmax_pitched")

    def corr_softargmax_il(self, l, r, out, batch, C, H, W, D, is_min, in_pitch=0, out_pitch=0, out_bstride=0, stream=None, out_slot=1):
        """out_slot = 4: the map as lane 0 of the 16-byte slots of an interleaved group, (H, out_pitch, 4), zeros in lanes 1..3"""
        self.check(self.lib.rt_corr_softargmax_il_slot(_ptr(l), _ptr(r), _ptr(out), batch, C, H, W, D, int(is_min), in_pitch, out_pitch,
                                                       out_bstride, out_slot, stream), "rt_corr_softargmax_il_slot")

    def corr_softargmax_il8_f16(self, l, r, out, batch, C, H, W, D, is_min, in_pitch=0, out_pitch=0, out_bstride=0, stream=None, out_slot=1):
        """half2 mode: fp16 (C/8, H, pitch, 8) feature maps, fp16 map out (out_slot = 8: lane 0 of the 16-byte slots of a group of 8)"""
        self.check(self.lib.rt_corr_softargmax_il8_f16(_ptr(l), _ptr(r), _ptr(out), batch, C, H, W, D, int(is_min), in_pitch, out_pitch,
                                                       out_bstride, out_slot, stream), "rt_corr_softargmax_il8_f16")

    def cost_volume(self, l, r, cv, batch, C, H, W, D, dtype=RT_F32, stream=None):
        self.check(self.lib.rt_cost_volume(_ptr(l), _ptr(r), _ptr(cv), batch, C, H, W, D, dtype, stream),
                   "rt_cost_volume")

    def softargmax(self, vol, out, batch, D, H, W, is_min, dtype=RT_F32, stream=None):
        self.check(self.lib.rt_softargmax(_ptr(vol), _ptr(out), batch, D, H, W, int(is_min), dtype, stream),
                   "rt_softargmax")

    def corr_softargmax(self, l, r, out, batch, C, H, W, D, is_min, out_bstride=0, dtype=RT_F32, stream=None, flags=0):
        self.check(self.lib.rt_corr_softargmax_flags(_ptr(l), _ptr(r), _ptr(out), batch, C, H, W, D, int(is_min), out_bstride, dtype,
                                                     flags, stream)
                   if flags else self.lib.rt_corr_softargmax(_ptr(l), _ptr(r), _ptr(out), batch, C, H, W, D, int(is_min),
                                                             out_bstride, dtype, stream), "rt_corr_softargmax")

    def permute4d(self, x, y, batch, dims, order, dtype=RT_F32, stream=None):
        o = (c_int * 4)(*order)
        self.check(self.lib.rt_permute4d(_ptr(x), _ptr(y), batch, dims[0], dims[1], dims[2], dims[3], o, dtype,
                                         stream), "rt_permute4d")

    def pad_d(self, x, y, batch, D, inner, pad_end, dtype=RT_F32, stream=None):
        self.check(self.lib.rt_pad_d(_ptr(x), _ptr(y), batch, D, inner, pad_end, dtype, stream), "rt_pad_d")

    def slice_d(self, x, y, batch, D, inner, start, end, dtype=RT_F32, stream=None):
        self.check(self.lib.rt_slice_d(_ptr(x), _ptr(y), batch, D, inner, start, end, dtype, stream), "rt_slice_d")

    def concat_channels(self, x, y, batch, C, Ctot, c_off, inner, dtype=RT_F32, stream=None):
        self.check(self.lib.rt_concat_channels(_ptr(x), _ptr(y), batch, C, Ctot, c_off, inner, dtype, stream),
                   "rt_concat_channels")

    # -- convolution plans -------------------------------------------------------------------------
    def has_experimental(self):
        """the library carries the rejected kernel families (RT_EXPERIMENTAL build: the emulator library of the CPU test tier)"""
        return bool(self.lib.rt_has_experimental())

    def disparity_to_color(self, disp_px, batch, h, w, max_disp, dst_rgb8, dst_step=None, stream=None):
        """(N,1,h,w) fp32 disparity in pixels -> rgb8 in the KITTI colour scheme, rows dst_step (default 3 w) bytes apart"""
        self.check(self.lib.rt_disparity_to_color(_ptr(disp_px), batch, h, w, max_disp, _ptr(dst_rgb8), 3 * w if dst_step is None else dst_step,
                                                  stream), "rt_disparity_to_color")

    def viz_mosaic_u8(self, left, right, src_h, src_w, src_step, encoding, disp_px, h, w, max_disp, dst_rgb8, dst_step=None, batch=1,
                      stream=None):
        """the viz node's 2x2 panel: frames as for preprocess_frames_u8 and their (N,1,h,w) disparity in pixels -> per image a 2h x 2w rgb8
        picture, rows dst_step (default 6 w) bytes apart: left | right over grey disparity | KITTI-coloured disparity"""
        self.check(self.lib.rt_viz_mosaic_u8(_ptr(left), _ptr(right), src_h, src_w, src_step, encoding, _ptr(disp_px), h, w, max_disp,
                                             _ptr(dst_rgb8), 6 * w if dst_step is None else dst_step, batch, stream), "rt_viz_mosaic_u8")

    def check_range(self, x, rows, valid, pitch, dtype=RT_F32, limit=65504.0, stream=None):
        """(max |x|, number of elements with |x| >= limit or non-finite) over `rows` rows of `valid` leading elements, `pitch` apart, of a
        device tensor (rt_check_range); max |x| is +inf as soon as one of them is inf or NaN"""
        mx, bad = c_float(), c_int64()
        self.check(self.lib.rt_check_range(_ptr(x), rows, valid, pitch, dtype, limit, ctypes.byref(mx), ctypes.byref(bad), stream), "rt_check_range")
        return mx.value, bad.value

    def convert_format(self, x, y, batch, C, inner, src_kind, dst_kind, stream=None):
        """(batch, C, inner) tensor between the forms of a plugin boundary (rt_convert_format): kinds 0 fp32 NCHW, 1 fp16 NCHW,
        2 fp16 NC2HW2 (channel pairs of a pixel in one 4-byte slot, an odd C zero padded)"""
        self.check(self.lib.rt_convert_format(_ptr(x), _ptr(y), batch, C, inner, src_kind, dst_kind, stream), "rt_convert_format")

    def hash_buffer(self, x, bytes, stream=None):
        """the 64-bit checksum of `bytes` (a multiple of 4) bytes of a device buffer (rt_hash_buffer), read back to the host"""
        out, value = c_void_p(), ctypes.c_uint64()
        self.check(self.lib.rt_malloc(ctypes.byref(out), 8), "rt_malloc")
        try:
            self.check(self.lib.rt_hash_buffer(_ptr(x), bytes, out, stream), "rt_hash_buffer")
            self.check(self.lib.rt_memcpy_d2h(ctypes.byref(value), out, 8, stream), "rt_memcpy_d2h")
            self.check(self.lib.rt_stream_sync(stream), "rt_stream_sync")
        finally:
            self.lib.rt_free(out)
        return value.value

    def conv2d_plan(self, w_host, b_host, Cin, Cout, Hin, Win, k, stride, pad, act=0, has_residual=False,
                    dtype=RT_F32, transposed=False, flags=0):
        d = Conv2dDesc(Cin, Cout, Hin, Win, k, k, stride, pad, pad, act, int(has_residual), dtype, flags)
        _host_weights(w_host, dtype, "conv2d_plan weights"); _host_weights(b_host, dtype, "conv2d_plan bias")
        plan = c_void_p()
        fn = self.lib.rt_deconv2d_plan_create if transposed else self.lib.rt_conv2d_plan_create
        self.check(fn(ctypes.byref(plan), ctypes.byref(d), _ptr(w_host), _ptr(b_host)), "conv2d plan")
        return ConvPlan(self, plan)

    def resblock_plan(self, w1, b1, w2, b2, C, Cmid, H, W, act1=RT_ACT_ELU, act2=RT_ACT_ELU, dtype=RT_F32):
        """fused residual block y = act2(conv3x3(act1(conv3x3(x) + b1)) + b2 + x)"""
        d1 = Conv2dDesc(C, Cmid, H, W, 3, 3, 1, 1, 1, act1, 0, dtype)
        d2 = Conv2dDesc(Cmid, C, H, W, 3, 3, 1, 1, 1, act2, 1, dtype)
        plan = c_void_p()
        self.check(self.lib.rt_resblock_plan_create(ctypes.byref(plan), ctypes.byref(d1), _ptr(w1), _ptr(b1), ctypes.byref(d2),
                                                    _ptr(w2), _ptr(b2)), "resblock plan")
        return ConvPlan(self, plan)

    def conv3d_plan(self, w_host, b_host, C, K, dims, kernel, stride, pad_start, pad_end, act=0, out_dchw=False,
                    has_residual=False, dtype=RT_F32, transposed_in_dims=None, out_depth=0, in_pad_end=0, cv_fold=0):
        d = Conv3dDesc(C, K, dims[0], dims[1], dims[2], (c_int * 3)(*kernel), (c_int * 3)(*stride),
                       (c_int * 3)(*pad_start), (c_int * 3)(*pad_end), act, int(out_dchw), int(has_residual), dtype,
                       out_depth, in_pad_end, cv_fold)
        plan = c_void_p()
        if transposed_in_dims is None:
            rc = self.lib.rt_conv3d_plan_create(ctypes.byref(plan), ctypes.byref(d), _ptr(w_host), _ptr(b_host))
        else:
            ind = (c_int * 3)(*transposed_in_dims)
            rc = self.lib.rt_conv3d_transpose_plan_create(ctypes.byref(plan), ctypes.byref(d), ind, _ptr(w_host),
                                                          _ptr(b_host))
        self.check(rc, "conv3d plan")
        return ConvPlan(self, plan)


class ConvPlan:
    def __init__(self, klib, handle):
        self.klib, self.handle = klib, handle
        dims = (c_int * 4)()
        klib.check(klib.lib.rt_conv_plan_out_dims(handle, dims), "rt_conv_plan_out_dims")
        self.out_dims = tuple(dims)

    def set_pitch(self, in_pitch, out_pitch):
        self.klib.check(self.klib.lib.rt_conv_plan_set_pitch(self.handle, in_pitch, out_pitch), "rt_conv_plan_set_pitch")

    def set_batch_strides(self, x_bstride, y_bstride, r_bstride=0):
        """per-sample strides in elements of input / output / residual (0 = leave as it is)"""
        self.klib.check(self.klib.lib.rt_conv_plan_set_batch_strides(self.handle, x_bstride, y_bstride, r_bstride), "rt_conv_plan_set_batch_strides")

    def set_io_types(self, x_dtype, y_dtype):
        self.klib.check(self.klib.lib.rt_conv_plan_set_io_types(self.handle, x_dtype, y_dtype), "rt_conv_plan_set_io_types")

    def input_limit(self):
        """bound on |x| the plan's arithmetic needs (65504 for fp16-pipe plans, inf for exact fp32)"""
        v = c_float()
        self.klib.check(self.klib.lib.rt_conv_plan_input_limit(self.handle, ctypes.byref(v)), "rt_conv_plan_input_limit")
        return v.value

    def supports_il8(self):
        return bool(self.klib.lib.rt_conv_plan_supports_il8(self.handle))

    def il_caps(self):
        """which tensors may be channel-interleaved: bit 0 input, bit 1 output, bit 2 residual, bit 3 output only with an interleaved input,
        bit 4 input with its channel count padded to a whole group"""
        return int(self.klib.lib.rt_conv_plan_supports_il8(self.handle))

    def set_layouts(self, x_il8, y_il8, r_il8=False):
        """channel-interleaved (C/8, H, pitch, 8) fp16 tensors: input / output / residual"""
        self.klib.check(self.klib.lib.rt_conv_plan_set_layouts(self.handle, int(x_il8), int(y_il8), int(r_il8)), "rt_conv_plan_set_layouts")

    def enqueue_twin_input(self, x, x2, y, batch=1, stream=None, hints=0):
        """first layer of both towers: samples [0, batch) from x, [batch, 2 batch) from x2"""
        self.klib.check(self.klib.lib.rt_conv_enqueue_twin_input(self.handle, _ptr(x), _ptr(x2), _ptr(y), batch, stream, hints), "rt_conv_enqueue_twin_input")

    def supports_split(self):
        return bool(self.klib.lib.rt_resblock_plan_supports_split(self.handle))

    def set_split(self, x_split, y_split):
        """pre-split tensors (C/8, H, pitch, [8 hi | 8 lo]) as input / output of a tower block"""
        self.klib.check(self.klib.lib.rt_resblock_plan_set_split(self.handle, int(x_split), int(y_split)), "rt_resblock_plan_set_split")

    def set_softarg(self, mode):
        """end the launch in the soft-argmax (1) / soft-argmin (2) over the output depth (last Conv3DTranspose of a 3-D model): y becomes the
        (batch, 1, H, W) map; raises RtError (RT_E_UNSUPPORTED) for a plan that has no such form"""
        self.klib.check(self.klib.lib.rt_conv_plan_set_softarg(self.handle, int(mode)), "rt_conv_plan_set_softarg")

    def enqueue(self, x, y, residual=None, batch=1, stream=None, hints=0):
        self.klib.check(self.klib.lib.rt_conv_enqueue_hint(self.handle, _ptr(x), _ptr(y), _ptr(residual), batch, stream, hints),
                        "rt_conv_enqueue")

    def destroy(self):
        if self.handle:
            self.klib.lib.rt_conv_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------
# whole-network ABI (include/rt_stereo_net.h, libnvstereo_inference.so)
# ---------------------------------------------------------------------------------------------------
RT_MODEL_RESNET18_2D, RT_MODEL_NVSMALL, RT_MODEL_NVTINY, RT_MODEL_RESNET18 = 0, 1, 2, 3
RT_RESIZE_AREA_DOWN, RT_RESIZE_CV_AREA = 0, 1                         # rtFrameCall.resize
RT_GEOM_NET, RT_GEOM_FRAME = 0, 1                                     # rtFrameCall.geometry
MODEL_IDS = {"resnet18_2D": RT_MODEL_RESNET18_2D, "nvsmall": RT_MODEL_NVSMALL, "nvtiny": RT_MODEL_NVTINY,
             "resnet18": RT_MODEL_RESNET18}

NET_SYMBOLS = {
    "rt_net_create": (c_int, [POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int, c_char_p]),
    "rt_net_create_from_memory": (c_int, [POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                          c_size_t]),
    "rt_net_serialize": (c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]),
    "rt_net_create_from_plan": (c_int, [POINTER(c_void_p), c_void_p, c_size_t]),
    "rt_net_execute": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "rt_net_execute_frames": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_int, c_int, c_void_p]),
    "rt_net_execute_frames_lr": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                         c_void_p, c_float, c_int, c_void_p]),
    "rt_net_execute_frames_viz": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_int64, c_float,
                                          c_float, c_void_p, c_void_p, c_int, c_void_p]),
    "rt_net_execute_frames_ex": (c_int, [c_void_p, c_void_p, c_void_p]),
    "rt_net_execute_frames_3d": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_net_execute_frames_raw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_net_execute_frames_filtered": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_net_execute_frames_camera": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_net_execute_frames_voxels": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_net_profile": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_char_p, c_size_t]),
    "rt_net_num_layers": (c_int, [c_void_p]),
    "rt_net_num_launches": (c_int, [c_void_p]),
    "rt_net_set_streams": (c_int, [c_void_p, c_int]),
    "rt_net_set_graph": (c_int, [c_void_p, c_int]),
    "rt_net_create_broadcast": (c_int, [POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int]),
    "rt_net_weights_crc32": (c_int, [c_void_p, POINTER(ctypes.c_uint32)]),
    "rt_net_weights_image": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_size_t)]),
    "rt_net_create_opt": (c_int, [POINTER(c_void_p), c_void_p]),
    "rt_net_set_debug": (c_int, [c_void_p, c_int]),
    "rt_net_set_launch_trace": (c_int, [c_void_p, c_int]),
    "rt_net_read_launch_trace": (c_int, [c_void_p, POINTER(ctypes.c_ulonglong), c_int]),
    "rt_net_launch_name": (c_char_p, [c_void_p, c_int]),
    "rt_net_read_launch_output": (ctypes.c_longlong, [c_void_p, c_int, c_void_p, ctypes.c_longlong]),
    "rt_net_destroy": (c_int, [c_void_p]),
    "rt_net_last_error": (c_char_p, []),
}


class NetOptions(ctypes.Structure):
    """rtNetOptions (include/rt_stereo_net.h)"""
    _fields_ = [("model", c_int), ("width", c_int), ("height", c_int), ("max_batch", c_int), ("weights_dtype", c_int), ("max_disp", c_int),
                ("weights_path", c_char_p), ("blob", c_void_p), ("bytes", c_size_t), ("flags", ctypes.c_uint), ("comm", c_void_p), ("root", c_int)]


class FrameCall(ctypes.Structure):
    """rtFrameCall (include/rt_stereo_net.h)"""
    _fields_ = [("struct_bytes", c_size_t), ("left_u8", c_void_p), ("right_u8", c_void_p), ("src_h", c_int), ("src_w", c_int),
                ("src_step", c_int64), ("encoding", c_int), ("resize", c_int), ("disp", c_void_p), ("disp_kind", c_int), ("geometry", c_int),
                ("max_diff_px", c_float), ("mask_u8", c_void_p), ("valid_count", c_void_p), ("batch", c_int)]


class DepthCall(ctypes.Structure):
    """rtDepthCall (include/rt_stereo_net.h)"""
    _fields_ = [("struct_bytes", c_size_t), ("camera", StereoCamera), ("min_depth", c_float), ("max_depth", c_float), ("depth", c_void_p),
                ("depth_kind", c_int), ("points", c_void_p), ("points_compact", c_void_p), ("count", c_void_p)]


class RectifyCall(ctypes.Structure):
    """rtRectifyCall (include/rt_stereo_net.h)"""
    _fields_ = [("struct_bytes", c_size_t), ("left", RectifyCamera), ("right", RectifyCamera), ("left_rect_u8", c_void_p),
                ("right_rect_u8", c_void_p), ("rect_step", c_int64)]


class SpeckleCall(ctypes.Structure):
    """rtSpeckleCall (include/rt_stereo_net.h)"""
    _fields_ = [("struct_bytes", c_size_t), ("max_size", c_int), ("max_diff_px", c_float)]


class DecodeCall(ctypes.Structure):
    """rtDecodeCall (include/rt_stereo_net.h)"""
    _fields_ = [("struct_bytes", c_size_t), ("wire_encoding", c_int), ("left_color_u8", c_void_p), ("right_color_u8", c_void_p),
                ("color_step", c_int64)]


class VoxelCall(ctypes.Structure):
    """rtVoxelCall (include/rt_stereo_net.h)"""
    _fields_ = [("struct_bytes", c_size_t), ("grid", VoxelGrid), ("min_points", c_int), ("voxels", c_void_p), ("capacity", c_int),
                ("count", c_void_p), ("cell_u32", c_void_p), ("n_u32", c_void_p)]


def pack_weights(weights, fp16=False):
    """dict name -> array  ==>  bytes in trt_weights.bin layout (scripts/tensorrt_model_builder.py:52-60)."""
    import struct

    import numpy as np
    out = bytearray()
    for name, v in weights.items():
        flat = np.asarray(v).reshape(-1)
        out += name.encode() + b"\0" + struct.pack("<I", flat.size)
        out += flat.astype("<f2" if fp16 else "<f4").tobytes()
    return bytes(out)


def read_weights(path, fp16=False):
    """trt_weights.bin / trt_weights_fp16.bin -> dict name -> float32 array (inverse of pack_weights; the reader of
    sample_app/main.cpp:111-134: name, NUL, uint32 count, count elements)."""
    import struct

    import numpy as np
    raw = open(path, "rb").read()
    off, out = 0, {}
    dt = np.dtype("<f2") if fp16 else np.dtype("<f4")
    while off < len(raw):
        end = raw.index(b"\0", off)
        (cnt,) = struct.unpack_from("<I", raw, end + 1)
        out[raw[off:end].decode()] = np.frombuffer(raw, dtype=dt, count=cnt, offset=end + 5).astype(np.float32)
        off = end + 5 + cnt * dt.itemsize
    return out


class NetLib:
    """libnvstereo_inference.so: the NvInfer.h shim + plugins + executor, through the C ABI."""

    def __init__(self, host_path=None, kernels_path=None):
        self.kernels = KernelLib(kernels_path)          # loads (and checks) the kernel library first
        path = host_path or HOST_LIB
        if not os.path.exists(path):
            raise RtError("native library %s is missing -- run `python -m redtail_amd.build`" % path)
        self.lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in NET_SYMBOLS.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args

    def check(self, rc, what):
        if rc != 0:
            raise RtError("%s failed (%d): %s" % (what, rc, self.lib.rt_net_last_error().decode()))

    def create(self, model, width, height, max_batch=1, weights=None, weights_path=None, fp16_weights=False,
               max_disp=0, flags=0):
        h = c_void_p()
        dt = RT_F16 if fp16_weights else RT_F32
        mid = MODEL_IDS[model] if isinstance(model, str) else model
        if flags:                                          # options beyond the plain entries: rt_net_create_opt
            blob = None if weights_path is not None else (weights if isinstance(weights, (bytes, bytearray)) else pack_weights(weights, fp16_weights))
            keep = ctypes.create_string_buffer(bytes(blob), len(blob)) if blob is not None else None
            o = NetOptions(mid, width, height, max_batch, dt, max_disp, weights_path.encode() if weights_path else None,
                           ctypes.cast(keep, c_void_p) if keep is not None else None, len(blob) if blob is not None else 0, flags, None, 0)
            self.check(self.lib.rt_net_create_opt(ctypes.byref(h), ctypes.byref(o)), "rt_net_create_opt")
            return StereoNet(self, h, width, height)
        if weights_path is not None:
            rc = self.lib.rt_net_create(ctypes.byref(h), mid, width, height, max_batch, dt, max_disp,
                                        weights_path.encode())
        else:
            blob = weights if isinstance(weights, (bytes, bytearray)) else pack_weights(weights, fp16_weights)
            rc = self.lib.rt_net_create_from_memory(ctypes.byref(h), mid, width, height, max_batch, dt, max_disp,
                                                    blob, len(blob))
        self.check(rc, "rt_net_create")
        return StereoNet(self, h, width, height)

    # ---- multi-GPU start-up through the native RCCL entry (include/rt_stereo.h: rt_comm_*, rt_stereo_net.h: rt_net_create_broadcast)
    def comm_unique_id(self):
        """rank 0: the 128 bytes every other rank needs for comm_init_rank (ncclGetUniqueId)"""
        buf = ctypes.create_string_buffer(RT_COMM_ID_BYTES)
        self.kernels.check(self.kernels.lib.rt_comm_unique_id(buf), "rt_comm_unique_id")
        return buf.raw

    def comm_init_rank(self, world, rank, unique_id):
        """ncclCommInitRank on the current device (rt_set_device first); returns an opaque handle"""
        h = c_void_p()
        self.kernels.check(self.kernels.lib.rt_comm_init_rank(ctypes.byref(h), world, rank, unique_id), "rt_comm_init_rank")
        return h

    def comm_init_all(self, ndev, devices=None):
        """ncclCommInitAll: one communicator per device of THIS process (apps/stereo_throughput.cpp: one thread per device)"""
        comms = (c_void_p * ndev)()
        devs = (c_int * ndev)(*devices) if devices is not None else None
        self.kernels.check(self.kernels.lib.rt_comm_init_all(ctypes.cast(comms, POINTER(c_void_p)), ndev, devs), "rt_comm_init_all")
        return [c_void_p(comms[i]) for i in range(ndev)]

    def comm_destroy(self, comm):
        self.kernels.check(self.kernels.lib.rt_comm_destroy(comm), "rt_comm_destroy")

    def create_broadcast(self, model, width, height, comm, root=0, max_batch=1, blob=None, fp16_weights=False, max_disp=0):
        """every rank calls this; rank `root` passes the weight-file image, the others receive it over RCCL (ncclBroadcast)"""
        h = c_void_p()
        dt = RT_F16 if fp16_weights else RT_F32
        mid = MODEL_IDS[model] if isinstance(model, str) else model
        rc = self.lib.rt_net_create_broadcast(ctypes.byref(h), mid, width, height, max_batch, dt, max_disp, blob, len(blob) if blob else 0, comm, root)
        self.check(rc, "rt_net_create_broadcast")
        return StereoNet(self, h, width, height)

    def create_from_plan(self, plan, width, height):
        """IRuntime::deserializeCudaEngine on bytes returned by StereoNet.serialize()"""
        h = c_void_p()
        self.check(self.lib.rt_net_create_from_plan(ctypes.byref(h), plan, len(plan)), "rt_net_create_from_plan")
        return StereoNet(self, h, width, height)


class StereoNet:
    def __init__(self, netlib, handle, width, height):
        self.netlib, self.handle, self.width, self.height = netlib, handle, width, height

    @property
    def num_layers(self):
        return self.netlib.lib.rt_net_num_layers(self.handle)

    @property
    def num_launches(self):
        return self.netlib.lib.rt_net_num_launches(self.handle)

    def execute(self, left, right, disp, batch=1, stream=None):
        self.netlib.check(self.netlib.lib.rt_net_execute(self.handle, _ptr(left), _ptr(right), _ptr(disp), batch, stream),
                          "rt_net_execute")

    @staticmethod
    def _frame_geometry(what, left_u8, right_u8, encoding, batch, src_step, src_w):
        """(height, width, step) of a pair of frame batches: (N, H, W, C) -- dense, or a view of padded rows (the row stride is the step) --
        or (N, H, step) raw rows, for which src_w gives the width in pixels"""
        bpp = ENC_BYTES.get(encoding)
        if bpp is None:                              # the C entry refuses it too; the shape logic below needs the pixel size
            raise RtError("%s: unknown encoding %r" % (what, encoding))
        shapes = []
        for f in (left_u8, right_u8):
            shape = tuple(f.shape)
            strides = tuple(f.stride()) if hasattr(f, "stride") and callable(f.stride) else tuple(f.strides)     # torch: elements, numpy: bytes (uint8: same)
            if len(shape) == 4:
                if shape[3] != bpp or strides[3] != 1 or strides[2] != bpp:
                    raise ValueError("frames of shape (N,H,W,C) need C = %d bytes per pixel, dense within a row" % bpp)
                h, w, step = shape[1], shape[2], strides[1]
            elif len(shape) == 3:
                if src_w is None or strides[2] != 1:
                    raise ValueError("frames of shape (N,H,step) need src_w and rows of contiguous bytes")
                h, w, step = shape[1], src_w, strides[1]
            else:
                raise ValueError("frames must be (N,H,W,C) or (N,H,step) uint8")
            if shape[0] < batch or (batch > 1 and strides[0] != h * step):
                raise ValueError("frame batch must hold %d frames of %d rows of %d bytes back to back" % (batch, h, step))
            shapes.append((h, w, step))
        if shapes[0] != shapes[1]:
            raise ValueError("left and right frames differ in size or step: %r vs %r" % tuple(shapes))
        h, w, step = shapes[0]
        return h, w, step if src_step is None else src_step

    def execute_frames(self, left_u8, right_u8, encoding, disp, kind=RT_DISP_PIXELS_F32, batch=1, stream=None, src_step=None,
                       src_w=None):
        """rt_net_execute_frames: two batches of camera frames in, disparity out.  Frames are uint8 torch device tensors (numpy arrays under
        the emulator) of shape (N, H, W, C) -- dense, or a view of padded rows (the row stride is the step) -- or (N, H, step) raw rows, for
        which src_w gives the width in pixels.  kind: RT_DISP_NET / RT_DISP_PIXELS_F32 (fp32, (N,1,h,w)) or RT_DISP_KITTI_U16 (16-bit)."""
        h, w, step = self._frame_geometry("rt_net_execute_frames", left_u8, right_u8, encoding, batch, src_step, src_w)
        self.netlib.check(self.netlib.lib.rt_net_execute_frames(self.handle, _ptr(left_u8), _ptr(right_u8), h, w, step, encoding,
                                                                _ptr(disp), kind, batch, stream), "rt_net_execute_frames")

    def execute_frames_lr(self, left_u8, right_u8, encoding, disp, kind=RT_DISP_PIXELS_F32, mask=None, disp_right=None, valid_count=None,
                          max_diff_px=1.0, batch=1, stream=None, src_step=None, src_w=None):
        """rt_net_execute_frames_lr: execute_frames with a left-right consistency check (one engine pass at batch 2 * batch, which must
        fit max_batch).  disp: (N,1,h,w) in `kind`, inconsistent pixels 0; mask: uint8 (N,1,h,w), 255 = consistent; disp_right: the right
        view's disparity in `kind`; valid_count: N uint64 on the device (torch: int64).  Frames as for execute_frames."""
        h, w, step = self._frame_geometry("rt_net_execute_frames_lr", left_u8, right_u8, encoding, batch, src_step, src_w)
        self.netlib.check(self.netlib.lib.rt_net_execute_frames_lr(self.handle, _ptr(left_u8), _ptr(right_u8), h, w, step, encoding,
                                                                   _ptr(disp), kind, _ptr(mask), _ptr(disp_right), _ptr(valid_count),
                                                                   max_diff_px, batch, stream), "rt_net_execute_frames_lr")

    def execute_frames_viz(self, left_u8, right_u8, encoding, disp_px, viz_rgb8, viz_step=None, max_disp=96.0, max_diff_px=-1.0, mask=None,
                           valid_count=None, batch=1, stream=None, src_step=None, src_w=None):
        """rt_net_execute_frames_viz: execute_frames (max_diff_px < 0) or execute_frames_lr (max_diff_px >= 0) with RT_DISP_PIXELS_F32 into
        disp_px, then the viz node's 2h x 2w rgb8 panel of the same frames and that disparity into viz_rgb8, rows viz_step (default 6 w)
        bytes apart.  Frames as for execute_frames."""
        h, w, step = self._frame_geometry("rt_net_execute_frames_viz", left_u8, right_u8, encoding, batch, src_step, src_w)
        self.netlib.check(self.netlib.lib.rt_net_execute_frames_viz(self.handle, _ptr(left_u8), _ptr(right_u8), h, w, step, encoding,
                                                                    _ptr(disp_px), _ptr(viz_rgb8), 6 * self.width if viz_step is None else viz_step,
                                                                    max_disp, max_diff_px, _ptr(mask), _ptr(valid_count), batch, stream),
                          "rt_net_execute_frames_viz")

    def execute_frames_ex(self, left_u8, right_u8, encoding, disp, kind=RT_DISP_PIXELS_F32, geometry=RT_GEOM_FRAME, resize=RT_RESIZE_CV_AREA,
                          max_diff_px=-1.0, mask=None, valid_count=None, batch=1, stream=None, src_step=None, src_w=None, struct_bytes=None):
        """rt_net_execute_frames_ex: frames of any size in (resize = RT_RESIZE_CV_AREA; RT_RESIZE_AREA_DOWN refuses up-scaling as
        execute_frames does), disparity out in the network's geometry (RT_GEOM_NET: (N,1,h,w)) or in the frame's (RT_GEOM_FRAME:
        (N,1,src_h,src_w), the frame's pixels), with a left-right check when max_diff_px >= 0 (mask, valid_count in the geometry of disp;
        2 * batch must fit max_batch).  Frames as for execute_frames."""
        h, w, step = self._frame_geometry("rt_net_execute_frames_ex", left_u8, right_u8, encoding, batch, src_step, src_w)
        call = FrameCall(ctypes.sizeof(FrameCall) if struct_bytes is None else struct_bytes, _ptr(left_u8), _ptr(right_u8), h, w, step, encoding,
                         resize, _ptr(disp), kind, geometry, max_diff_px, _ptr(mask), _ptr(valid_count), batch)
        self.netlib.check(self.netlib.lib.rt_net_execute_frames_ex(self.handle, ctypes.byref(call), stream), "rt_net_execute_frames_ex")

    def execute_frames_3d(self, left_u8, right_u8, encoding, camera, disp=None, kind=RT_DISP_PIXELS_F32, geometry=RT_GEOM_FRAME,
                          resize=RT_RESIZE_CV_AREA, max_diff_px=-1.0, mask=None, valid_count=None, min_depth=0.0, max_depth=float("inf"),
                          depth=None, depth_kind=RT_DEPTH_M_F32, points=None, points_compact=None, count=None, batch=1, stream=None,
                          src_step=None, src_w=None, struct_bytes=None, depth_struct_bytes=None, no_depth_call=False):
        """rt_net_execute_frames_3d: execute_frames_ex in frame geometry with a depth image (N,1,src_h,src_w), the organised cloud
        (N,src_h,src_w) x 16 bytes and / or the compact cloud with its uint64 count per image beside (or, disp=None, instead of) the
        disparity.  camera: StereoCamera, the camera's own calibration at the frame's size.  no_depth_call: pass out = NULL."""
        h, w, step = self._frame_geometry("rt_net_execute_frames_3d", left_u8, right_u8, encoding, batch, src_step, src_w)
        call = FrameCall(ctypes.sizeof(FrameCall) if struct_bytes is None else struct_bytes, _ptr(left_u8), _ptr(right_u8), h, w, step, encoding,
                         resize, _ptr(disp), kind, geometry, max_diff_px, _ptr(mask), _ptr(valid_count), batch)
        out = None
        if not no_depth_call:
            out = ctypes.byref(DepthCall(ctypes.sizeof(DepthCall) if depth_struct_bytes is None else depth_struct_bytes,
                                         camera if camera is not None else StereoCamera(), min_depth, max_depth, _ptr(depth), depth_kind,
                                         _ptr(points), _ptr(points_compact), _ptr(count)))
        self.netlib.check(self.netlib.lib.rt_net_execute_frames_3d(self.handle, ctypes.byref(call), out, stream), "rt_net_execute_frames_3d")

    def execute_frames_raw(self, left_u8, right_u8, encoding, rect_left, rect_right, camera=None, disp=None, kind=RT_DISP_PIXELS_F32,
                           geometry=RT_GEOM_FRAME, resize=RT_RESIZE_CV_AREA, max_diff_px=-1.0, mask=None, valid_count=None, min_depth=0.0,
                           max_depth=float("inf"), depth=None, depth_kind=RT_DEPTH_M_F32, points=None, points_compact=None, count=None, batch=1,
                           stream=None, src_step=None, src_w=None, struct_bytes=None, depth_struct_bytes=None, no_depth_call=False,
                           left_rect=None, right_rect=None, rect_step=None, rect_struct_bytes=None):
        """rt_net_execute_frames_raw: RAW frames in.  One rectify_frames_u8 launch with the RectifyCameras rect_left / rect_right into
        rectified frames of the same size and encoding (buffers of the net, or left_rect / right_rect: (N, H, rect_step) uint8, rect_step
        defaulting to their row stride), then execute_frames_3d on them with the same keywords (no_depth_call: execute_frames_ex)."""
        h, w, step = self._frame_geometry("rt_net_execute_frames_raw", left_u8, right_u8, encoding, batch, src_step, src_w)
        call = FrameCall(ctypes.sizeof(FrameCall) if struct_bytes is None else struct_bytes, _ptr(left_u8), _ptr(right_u8), h, w, step, encoding,
                         resize, _ptr(disp), kind, geometry, max_diff_px, _ptr(mask), _ptr(valid_count), batch)
        out = None
        if not no_depth_call:
            out = ctypes.byref(DepthCall(ctypes.sizeof(DepthCall) if depth_struct_bytes is None else depth_struct_bytes,
                                         camera if camera is not None else StereoCamera(), min_depth, max_depth, _ptr(depth), depth_kind,
                                         _ptr(points), _ptr(points_compact), _ptr(count)))
        if rect_step is None:
            given = left_rect if left_rect is not None else right_rect
            rect_step = 0 if given is None else (given.stride(1) if hasattr(given, "data_ptr") else given.strides[1])
        rect = RectifyCall(ctypes.sizeof(RectifyCall) if rect_struct_bytes is None else rect_struct_bytes, rect_left, rect_right,
                           _ptr(left_rect), _ptr(right_rect), rect_step)
        self.netlib.check(self.netlib.lib.rt_net_execute_frames_raw(self.handle, ctypes.byref(call), out, ctypes.byref(rect), stream),
                          "rt_net_execute_frames_raw")

    def execute_frames_filtered(self, left_u8, right_u8, encoding, speckle_size=None, speckle_range=1.0, rect_left=None, rect_right=None,
                                camera=None, disp=None, kind=RT_DISP_PIXELS_F32, geometry=RT_GEOM_FRAME, resize=RT_RESIZE_CV_AREA,
                                max_diff_px=-1.0, mask=None, valid_count=None, min_depth=0.0, max_depth=float("inf"), depth=None,
                                depth_kind=RT_DEPTH_M_F32, points=None, points_compact=None, count=None, batch=1, stream=None, src_step=None,
                                src_w=None, struct_bytes=None, depth_struct_bytes=None, no_depth_call=False, left_rect=None, right_rect=None,
                                rect_step=None, rect_struct_bytes=None, speckle_struct_bytes=None):
        """rt_net_execute_frames_filtered: execute_frames_raw (rect_left / rect_right given), execute_frames_3d or (no_depth_call)
        execute_frames_ex with the same keywords, plus one disparity_speckle(speckle_size, speckle_range) in network geometry in front of
        the resampling; mask and valid_count are then legal without a check.  speckle_size=None: no filter, the wrapped call itself."""
        h, w, step = self._frame_geometry("rt_net_execute_frames_filtered", left_u8, right_u8, encoding, batch, src_step, src_w)
        call = FrameCall(ctypes.sizeof(FrameCall) if struct_bytes is None else struct_bytes, _ptr(left_u8), _ptr(right_u8), h, w, step, encoding,
                         resize, _ptr(disp), kind, geometry, max_diff_px, _ptr(mask), _ptr(valid_count), batch)
        out = None
        if not no_depth_call:
            out = ctypes.byref(DepthCall(ctypes.sizeof(DepthCall) if depth_struct_bytes is None else depth_struct_bytes,
                                         camera if camera is not None else StereoCamera(), min_depth, max_depth, _ptr(depth), depth_kind,
                                         _ptr(points), _ptr(points_compact), _ptr(count)))
        rect = None
        if rect_left is not None or rect_right is not None:
            if rect_step is None:
                given = left_rect if left_rect is not None else right_rect
                rect_step = 0 if given is None else (given.stride(1) if hasattr(given, "data_ptr") else given.strides[1])
            rect = ctypes.byref(RectifyCall(ctypes.sizeof(RectifyCall) if rect_struct_bytes is None else rect_struct_bytes, rect_left, rect_right,
                                            _ptr(left_rect), _ptr(right_rect), rect_step))
        speckle = None
        if speckle_size is not None:
            speckle = ctypes.byref(SpeckleCall(ctypes.sizeof(SpeckleCall) if speckle_struct_bytes is None else speckle_struct_bytes, speckle_size,
                                               speckle_range))
        self.netlib.check(self.netlib.lib.rt_net_execute_frames_filtered(self.handle, ctypes.byref(call), out, rect, speckle, stream),
                          "rt_net_execute_frames_filtered")

    def execute_frames_camera(self, left_wire, right_wire, wire_encoding, encoding=RT_ENC_BGR8, speckle_size=None, speckle_range=1.0,
                              rect_left=None, rect_right=None, camera=None, disp=None, kind=RT_DISP_PIXELS_F32, geometry=RT_GEOM_FRAME,
                              resize=RT_RESIZE_CV_AREA, max_diff_px=-1.0, mask=None, valid_count=None, min_depth=0.0, max_depth=float("inf"),
                              depth=None, depth_kind=RT_DEPTH_M_F32, points=None, points_compact=None, count=None, batch=1, stream=None,
                              src_step=None, src_w=None, struct_bytes=None, depth_struct_bytes=None, no_depth_call=False, left_rect=None,
                              right_rect=None, rect_step=None, rect_struct_bytes=None, speckle_struct_bytes=None, left_color=None,
                              right_color=None, color_step=None, decode_struct_bytes=None):
        """rt_net_execute_frames_camera: what the camera really sends in.  left_wire / right_wire: (N, H, step) uint8 rows of wire_encoding
        (RT_WIRE_*: mono8 / mono16, 8-bit Bayer, YUV 4:2:2; src_w defaults to step // bytes per wire pixel).  One decode_frames_u8 launch
        into colour frames of `encoding` (buffers of the net, or left_color / right_color: (N, H, color_step) uint8, color_step defaulting
        to their row stride), then execute_frames_filtered on them with the same keywords.  wire_encoding=None: no decode, `encoding`
        frames in, execute_frames_filtered itself."""
        strides = lambda t: tuple(t.stride()) if hasattr(t, "data_ptr") else tuple(t.strides)
        if wire_encoding is None:
            h, w, step = self._frame_geometry("rt_net_execute_frames_camera", left_wire, right_wire, encoding, batch, src_step, src_w)
        else:
            shape, st = tuple(left_wire.shape), strides(left_wire)
            if len(shape) != 3 or tuple(right_wire.shape) != shape or strides(right_wire) != st or st[2] != 1:
                raise ValueError("wire frames must be two (N,H,step) uint8 batches of the same shape, rows of contiguous bytes")
            if shape[0] < batch or (batch > 1 and st[0] != shape[1] * st[1]):
                raise ValueError("frame batch must hold %d frames of %d rows of %d bytes back to back" % (batch, shape[1], st[1]))
            h, step = shape[1], st[1] if src_step is None else src_step
            w = src_w if src_w is not None else shape[2] // WIRE_BYTES.get(wire_encoding, 1)
        call = FrameCall(ctypes.sizeof(FrameCall) if struct_bytes is None else struct_bytes, _ptr(left_wire), _ptr(right_wire), h, w, step, encoding,
                         resize, _ptr(disp), kind, geometry, max_diff_px, _ptr(mask), _ptr(valid_count), batch)
        out = None
        if not no_depth_call:
            out = ctypes.byref(DepthCall(ctypes.sizeof(DepthCall) if depth_struct_bytes is None else depth_struct_bytes,
                                         camera if camera is not None else StereoCamera(), min_depth, max_depth, _ptr(depth), depth_kind,
                                         _ptr(points), _ptr(points_compact), _ptr(count)))
        rect = None
        if rect_left is not None or rect_right is not None:
            if rect_step is None:
                given = left_rect if left_rect is not None else right_rect
                rect_step = 0 if given is None else strides(given)[1]
            rect = ctypes.byref(RectifyCall(ctypes.sizeof(RectifyCall) if rect_struct_bytes is None else rect_struct_bytes, rect_left, rect_right,
                                            _ptr(left_rect), _ptr(right_rect), rect_step))
        speckle = None
        if speckle_size is not None:
            speckle = ctypes.byref(SpeckleCall(ctypes.sizeof(SpeckleCall) if speckle_struct_bytes is None else speckle_struct_bytes, speckle_size,
                                               speckle_range))
        decode = None
        if wire_encoding is not None:
            if color_step is None:
                given = left_color if left_color is not None else right_color
                color_step = 0 if given is None else strides(given)[1]
            decode = ctypes.byref(DecodeCall(ctypes.sizeof(DecodeCall) if decode_struct_bytes is None else decode_struct_bytes, wire_encoding,
                                             _ptr(left_color), _ptr(right_color), color_step))
        self.netlib.check(self.netlib.lib.rt_net_execute_frames_camera(self.handle, ctypes.byref(call), out, rect, speckle, decode, stream),
                          "rt_net_execute_frames_camera")

    def execute_frames_voxels(self, left_u8, right_u8, encoding, grid=None, min_points=1, voxels=None, voxel_capacity=None, voxel_count=None,
                              voxel_cell=None, voxel_n=None, voxel_struct_bytes=None, speckle_size=None, speckle_range=1.0, rect_left=None,
                              rect_right=None, camera=None, disp=None, kind=RT_DISP_PIXELS_F32, geometry=RT_GEOM_FRAME, resize=RT_RESIZE_CV_AREA,
                              max_diff_px=-1.0, mask=None, valid_count=None, min_depth=0.0, max_depth=float("inf"), depth=None,
                              depth_kind=RT_DEPTH_M_F32, points=None, points_compact=None, count=None, batch=1, stream=None, src_step=None,
                              src_w=None, struct_bytes=None, depth_struct_bytes=None, no_depth_call=False, left_rect=None, right_rect=None,
                              rect_step=None, rect_struct_bytes=None, speckle_struct_bytes=None, wire_encoding=None, left_color=None,
                              right_color=None, color_step=None, decode_struct_bytes=None):
        """rt_net_execute_frames_voxels: execute_frames_filtered with the same keywords (and, wire_encoding given, execute_frames_camera's:
        left_u8 / right_u8 are then (N, H, step) wire frames), plus one points_voxel_grid(grid, min_points) behind the cloud: voxels
        (N, voxel_capacity) x 16 bytes -- voxel_capacity defaulting to the buffer's records per image --, voxel_count N uint64, voxel_cell /
        voxel_n (N, voxel_capacity) uint32.  No cloud output need be asked for.  grid=None: no voxel call, the wrapped call itself."""
        strides = lambda t: tuple(t.stride()) if hasattr(t, "data_ptr") else tuple(t.strides)
        if wire_encoding is None:
            h, w, step = self._frame_geometry("rt_net_execute_frames_voxels", left_u8, right_u8, encoding, batch, src_step, src_w)
        else:
            shape, st = tuple(left_u8.shape), strides(left_u8)
            if len(shape) != 3 or tuple(right_u8.shape) != shape or strides(right_u8) != st or st[2] != 1:
                raise ValueError("wire frames must be two (N,H,step) uint8 batches of the same shape, rows of contiguous bytes")
            if shape[0] < batch or (batch > 1 and st[0] != shape[1] * st[1]):
                raise ValueError("frame batch must hold %d frames of %d rows of %d bytes back to back" % (batch, shape[1], st[1]))
            h, step = shape[1], st[1] if src_step is None else src_step
            w = src_w if src_w is not None else shape[2] // WIRE_BYTES.get(wire_encoding, 1)
        call = FrameCall(ctypes.sizeof(FrameCall) if struct_bytes is None else struct_bytes, _ptr(left_u8), _ptr(right_u8), h, w, step, encoding,
                         resize, _ptr(disp), kind, geometry, max_diff_px, _ptr(mask), _ptr(valid_count), batch)
        out = None
        if not no_depth_call:
            out = ctypes.byref(DepthCall(ctypes.sizeof(DepthCall) if depth_struct_bytes is None else depth_struct_bytes,
                                         camera if camera is not None else StereoCamera(), min_depth, max_depth, _ptr(depth), depth_kind,
                                         _ptr(points), _ptr(points_compact), _ptr(count)))
        rect = None
        if rect_left is not None or rect_right is not None:
            if rect_step is None:
                given = left_rect if left_rect is not None else right_rect
                rect_step = 0 if given is None else strides(given)[1]
            rect = ctypes.byref(RectifyCall(ctypes.sizeof(RectifyCall) if rect_struct_bytes is None else rect_struct_bytes, rect_left, rect_right,
                                            _ptr(left_rect), _ptr(right_rect), rect_step))
        speckle = None
        if speckle_size is not None:
            speckle = ctypes.byref(SpeckleCall(ctypes.sizeof(SpeckleCall) if speckle_struct_bytes is None else speckle_struct_bytes, speckle_size,
                                               speckle_range))
        decode = None
        if wire_encoding is not None:
            if color_step is None:
                given = left_color if left_color is not None else right_color
                color_step = 0 if given is None else strides(given)[1]
            decode = ctypes.byref(DecodeCall(ctypes.sizeof(DecodeCall) if decode_struct_bytes is None else decode_struct_bytes, wire_encoding,
                                             _ptr(left_color), _ptr(right_color), color_step))
        voxel = None
        if grid is not None:
            if voxel_capacity is None:
                voxel_capacity = 0 if voxels is None else int(voxels.shape[1])
            voxel = ctypes.byref(VoxelCall(ctypes.sizeof(VoxelCall) if voxel_struct_bytes is None else voxel_struct_bytes, grid, min_points,
                                           _ptr(voxels), voxel_capacity, _ptr(voxel_count), _ptr(voxel_cell), _ptr(voxel_n)))
        self.netlib.check(self.netlib.lib.rt_net_execute_frames_voxels(self.handle, ctypes.byref(call), out, rect, speckle, decode, voxel, stream),
                          "rt_net_execute_frames_voxels")

    def set_debug(self, on=True):
        """IExecutionContext::setDebugSync: synchronise every launch and range-check the input of every fp16-pipe convolution"""
        self.netlib.check(self.netlib.lib.rt_net_set_debug(self.handle, int(on)), "rt_net_set_debug")

    def weights_crc32(self):
        """crc32 of the weight-file image this engine was built from (== zlib.crc32 of the file)"""
        c = ctypes.c_uint32()
        self.netlib.check(self.netlib.lib.rt_net_weights_crc32(self.handle, ctypes.byref(c)), "rt_net_weights_crc32")
        return c.value

    def weights_image(self):
        """bytes of the weight-file image the engine holds (what a non-root rank received by broadcast)"""
        p, n = c_void_p(), c_size_t()
        self.netlib.check(self.netlib.lib.rt_net_weights_image(self.handle, ctypes.byref(p), ctypes.byref(n)), "rt_net_weights_image")
        return ctypes.string_at(p.value, n.value)

    def set_launch_trace(self, on=True):
        """hash every launch's output on its own stream (debugging aid): read_launch_trace() after a pass"""
        self.netlib.check(self.netlib.lib.rt_net_set_launch_trace(self.handle, int(on)), "rt_net_set_launch_trace")

    def read_launch_trace(self):
        n = self.num_launches
        buf = (ctypes.c_ulonglong * n)()
        got = self.netlib.lib.rt_net_read_launch_trace(self.handle, buf, n)
        if got < 0:
            raise RtError("rt_net_read_launch_trace failed: " + self.netlib.lib.rt_net_last_error().decode())
        return list(buf[:got])

    def launch_name(self, i):
        s = self.netlib.lib.rt_net_launch_name(self.handle, i)
        return s.decode() if s else None

    def read_launch_output(self, i):
        """raw bytes of launch i's output tensor as stored on the device (numpy uint8 array)"""
        import numpy as np
        n = self.netlib.lib.rt_net_read_launch_output(self.handle, i, None, 0)
        if n < 0:
            raise RtError("rt_net_read_launch_output failed: " + self.netlib.lib.rt_net_last_error().decode())
        out = np.empty(n, np.uint8)
        if self.netlib.lib.rt_net_read_launch_output(self.handle, i, out.ctypes.data, n) != n:
            raise RtError("rt_net_read_launch_output failed: " + self.netlib.lib.rt_net_last_error().decode())
        return out

    def set_streams(self, n):
        """1: all launches on the caller's stream (throughput with several contexts); 2: second stream for the right encoder"""
        self.netlib.check(self.netlib.lib.rt_net_set_streams(self.handle, n), "rt_net_set_streams")

    def set_graph(self, on):
        """graph mode: repeated executes with the same pointers replay one captured hipGraph (rt_net_set_graph)"""
        self.netlib.check(self.netlib.lib.rt_net_set_graph(self.handle, int(bool(on))), "rt_net_set_graph")

    def profile(self, left, right, disp, batch=1):
        buf = ctypes.create_string_buffer(1 << 16)
        self.netlib.check(self.netlib.lib.rt_net_profile(self.handle, _ptr(left), _ptr(right), _ptr(disp), batch, buf,
                                                         len(buf)), "rt_net_profile")
        rows = []
        for line in buf.value.decode().splitlines():
            name, ms = line.rsplit("\t", 1)
            rows.append((name, float(ms)))
        return rows

    def serialize(self):
        """engine plan bytes (ICudaEngine::serialize)"""
        n = ctypes.c_size_t()
        self.netlib.check(self.netlib.lib.rt_net_serialize(self.handle, None, 0, ctypes.byref(n)), "rt_net_serialize")
        buf = ctypes.create_string_buffer(n.value)
        self.netlib.check(self.netlib.lib.rt_net_serialize(self.handle, buf, n.value, ctypes.byref(n)), "rt_net_serialize")
        return buf.raw

    def destroy(self):
        if self.handle:
            self.netlib.lib.rt_net_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
