/*
 * rt_stereo.h -- thin C ABI over the MI355X (gfx950) HIP kernels of the Stereo DNN hot path.
 *
 * This is the drop-in boundary "host C++ calls HIP through": every plugin `enqueue` in
 * redtail_amd/csrc/host/plugins.cpp and every TensorRT-native layer of the shim executor ends in
 * exactly one of these entry points.  Plain pointers, ints and an opaque stream handle only -- no
 * torch, HIP or C++ types -- so the same functions bind from C++, ctypes, cgo, JNI ...
 * (see INTEGRATION.md).  Each entry cites the reference interface it replaces
 * (paths relative to /root/reference/stereoDNN).
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers; tensors are dense, row-major, batch outermost;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value 0 = success; >0 = hipError_t from the runtime; <0 = RT_E_* argument errors.
 *     rt_last_error_string() describes the last failure of the calling thread
 *     (reference convention: enqueue returns 0 / non-zero, lib/cost_volume_plugin.cpp:138);
 *   - dtype: RT_F32 everywhere; RT_F16 where noted (fp16 storage, fp32 accumulate, as the
 *     reference does in lib/kernels.cu:218-223).
 */
#ifndef RT_STEREO_H
#define RT_STEREO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rtStream;

enum { RT_F32 = 0, RT_F16 = 1 };                     /* nvinfer1::DataType kFLOAT / kHALF            */
enum { RT_NCHW = 0, RT_NC2HW2 = 1 };                 /* nvinfer1::PluginFormat                       */
enum { RT_ACT_NONE = 0, RT_ACT_ELU = 1, RT_ACT_SIGMOID = 2 };
enum { RT_E_BADARG = -1, RT_E_UNSUPPORTED = -2, RT_E_NODEVICE = -3, RT_E_NOMEM = -4, RT_E_RUNTIME = -5 };

/* ---- library / device ------------------------------------------------------------------- */
const char* rt_last_error_string(void);
const char* rt_backend_name(void);                   /* "hip:gfx950 (<device name>)"                 */
int rt_device_count(void);
int rt_set_device(int ordinal);

/* Device memory, copies, streams and timing, so that a host library needs no HIP headers
 * (replaces the cudaMalloc / cudaMemcpy / cudaStream / cudaEvent calls in
 * sample_app/main.cpp:295-315 and lib/conv3d_plugin.cpp:122-133). */
int rt_malloc(void** dptr, size_t bytes);
int rt_free(void* dptr);
int rt_memcpy_h2d(void* dst, const void* src, size_t bytes, rtStream stream);
int rt_memcpy_d2h(void* dst, const void* src, size_t bytes, rtStream stream);
int rt_memcpy_d2d(void* dst, const void* src, size_t bytes, rtStream stream);
int rt_memset(void* dst, int value, size_t bytes, rtStream stream);
int rt_stream_create(rtStream* stream);             /* non-blocking w.r.t. the NULL stream */
int rt_stream_destroy(rtStream stream);
int rt_stream_sync(rtStream stream);
int rt_stream_wait_event(rtStream stream, void* ev);   /* later work on `stream` waits for `ev` */
int rt_event_create(void** ev);
int rt_event_create_ordering(void** ev);              /* no timestamps: for rt_stream_wait_event only (cudaEventDisableTiming) */
int rt_event_destroy(void* ev);
int rt_event_record(void* ev, rtStream stream);
int rt_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* synchronises on ev_stop */
/* hipGraph of everything issued on `stream` (and on streams that join it through events) between begin and end: an executor
 * captures one pass over fixed bindings and replays it with ONE rt_graph_launch (TensorRT's enqueue is graph-capturable the same
 * way; cudaStreamBeginCapture / cudaGraphInstantiate / cudaGraphLaunch).  Relaxed capture mode; RT_E_UNSUPPORTED on the emulator. */
typedef struct rtGraph rtGraph;
int rt_graph_begin_capture(rtStream stream);
int rt_graph_end_capture(rtStream stream, rtGraph** graph);          /* ends the capture and instantiates; NULL graph on failure */
int rt_graph_launch(rtGraph* graph, rtStream stream);
int rt_graph_destroy(rtGraph* graph);

/* ---- element-wise ------------------------------------------------------------------------ */
/* ELU, alpha = 1: y = x > 0 ? x : exp(x) - 1.  Replaces EluPlugin::enqueue ->
 * cudnnActivationForward (lib/elu_plugin.cpp:123-135).  n = element count (any layout: for
 * kNC2HW2 pass the padded count, lib/elu_plugin.cpp:165-168).  In-place allowed. */
int rt_elu(const void* x, void* y, int64_t n, int dtype, rtStream stream);

/* y = act(a + b) -- TensorRT addElementWise(kSUM) (+ a following ELU plugin when fused),
 * e.g. sample_app/resnet18_2D_513x257_net.cpp:95-103.  In-place allowed. */
int rt_add_act(const void* a, const void* b, void* y, int64_t n, int act, int dtype, rtStream stream);

/* y = act(x) for RT_ACT_SIGMOID / RT_ACT_ELU -- addActivation(kSIGMOID),
 * sample_app/resnet18_2D_513x257_net.cpp:766. */
int rt_activation(const void* x, void* y, int64_t n, int act, int dtype, rtStream stream);

/* ---- cost volumes ------------------------------------------------------------------------ */
/* Correlation cost volume: cv[n,d,y,x] = sum_c L[n,c,y,x] * R[n,c,y,x-d], 0 for x < d.
 * left/right (N,C,H,W) -> cv (N,D,H,W).  Replaces CudaKernels::computeCorrCostVolume /
 * corrCostVolumeKernel (lib/kernels.cu:168-200,252-287).  RT_F16 + RT_NC2HW2 follows
 * corrCostVolumeFP16NC2HW2Kernel (lib/kernels.cu:203-250): channel pairs packed in 32-bit
 * words, fp32 accumulate, output planes packed in disparity pairs. */
int rt_corr_cost_volume(const void* left, const void* right, void* cost_vol, int batch, int C, int H, int W,
                        int max_disp, int dtype, int format, rtStream stream);
/* The same with flags.  fp32 NCHW maps of a network's size (W >= 64, 16 <= C <= 32, max_disp <= 64) are correlated on the matrix
 * cores through the 3-term fp16 split of the convolutions (relative error <= 2^-21 of sum |l r|, inputs |x| < 65504);
 * RT_CONV_EXACT_FP32 keeps the fp32 fmaf chain of corrCostVolumeKernel for them too (CostVolumePlugin::enqueue passes it in engines
 * built with IBuilder::setExactFp32Mode). */
int rt_corr_cost_volume_flags(const void* left, const void* right, void* cost_vol, int batch, int C, int H, int W,
                              int max_disp, int dtype, int format, unsigned flags, rtStream stream);

/* Default (concatenation) cost volume: cv[n,d,0:C]=L ; cv[n,d,C:2C,y,x]=R[n,:,y,x-d] (0 for x<d).
 * (N,C,H,W) x2 -> (N,D,2C,H,W).  Replaces CudaKernels::computeCostVolume (lib/kernels.cu:50-97,136-161). */
int rt_cost_volume(const void* left, const void* right, void* cost_vol, int batch, int C, int H, int W,
                   int max_disp, int dtype, rtStream stream);

/* Soft-argmax (is_min = 0) / soft-argmin (1): out[n,y,x] = sum_d d * softmax_d(+-vol[n,d,y,x]).
 * vol (N,D,H,W) -> out (N,1,H,W), one pass, no workspace.  Replaces SoftargmaxPlugin::enqueue
 * (5 cuDNN/memcpy passes over a 2x workspace, lib/softargmax_plugin.cpp:167-205). */
int rt_softargmax(const void* vol, void* out, int batch, int D, int H, int W, int is_min, int dtype,
                  rtStream stream);

/* Fused correlation cost volume + soft-argmax/min: the D-volume never reaches HBM.
 * out element (n,y,x) is written at out + n*out_batch_stride + y*W + x (elements), which lets the
 * caller place the result directly in a channel of a concatenation buffer
 * (sample_app/resnet18_2D_513x257_net.cpp:601-615). */
int rt_corr_softargmax(const void* left, const void* right, void* out, int batch, int C, int H, int W,
                       int max_disp, int is_min, int64_t out_batch_stride, int dtype, rtStream stream);
/* (fp32 maps of a network's size -- W >= 64, 16 <= C <= 32, max_disp <= 64 -- are correlated on the matrix cores through the 3-term fp16
 * split of the convolutions; smaller ones by the fp32 fmaf chain of the reference kernel.)  Domain of that default path: every feature
 * value |x| < 65504 (the fp16 range of the high part; rt_check_range checks it).  Outside it the result is inf or NaN where the fp32
 * chain is finite -- a caller whose maps may leave the range passes RT_CONV_EXACT_FP32 to rt_corr_softargmax_flags.
 * The same with flags: RT_CONV_EXACT_FP32 keeps the fp32 fmaf chain for maps of every size. */
int rt_corr_softargmax_flags(const void* left, const void* right, void* out, int batch, int C, int H, int W,
                             int max_disp, int is_min, int64_t out_batch_stride, int dtype, unsigned flags, rtStream stream);
/*
 * Same with row pitches (elements, 0 = dense) for the feature maps and for the output plane; see
 * rt_conv_plan_set_pitch.  This entry always computes the fp32 chain: it is what engines built with
 * IBuilder::setExactFp32Mode call. */
int rt_corr_softargmax_pitched(const void* left, const void* right, void* out, int batch, int C, int H, int W,
                               int max_disp, int is_min, int in_pitch, int out_pitch, int64_t out_batch_stride,
                               int dtype, rtStream stream);
/* The same fused correlation + soft-argmax on channel-interleaved (C/4, H, pitch, 4) fp32 feature maps -- the executor's
 * internal layout between 3x3 convolutions -- computed on the matrix cores (C a multiple of 4 up to 32, D <= 64). */
int rt_corr_softargmax_il(const void* left, const void* right, void* out, int batch, int C, int H, int W, int D,
                          int is_min, int in_pitch, int out_pitch, int64_t out_bstride, rtStream stream);
/* ... with the map written as lane 0 of the 16-byte pixel slots of a channel-interleaved group, (H, out_pitch, 4) with zeros in
 * lanes 1..3 (out_slot = 4; 1 = the plane above): the disparity channel of conv2D_1's 33-channel input when the executor keeps
 * that concatenation interleaved (sample_app/resnet18_2D_513x257_net.cpp:601-615). */
int rt_corr_softargmax_il_slot(const void* left, const void* right, void* out, int batch, int C, int H, int W, int D,
                               int is_min, int in_pitch, int out_pitch, int64_t out_bstride, int out_slot, rtStream stream);
/* ... in half2 mode: fp16 channel-interleaved feature maps (C/8, H, pitch, 8), the map as an fp16 plane; the stored values are the
 * operands of the matrix instructions (fp32 accumulation of exact fp16 products, lib/kernels.cu:203-250 computes the same in fp32).
 * out_slot = 8: the map as lane 0 of the 16-byte slots of an interleaved group of 8 fp16 channels, zeros in lanes 1 .. 7. */
int rt_corr_softargmax_il8_f16(const void* left, const void* right, void* out, int batch, int C, int H, int W, int D,
                               int is_min, int in_pitch, int out_pitch, int64_t out_bstride, int out_slot, rtStream stream);

/* ---- layout glue of the 3-D models ------------------------------------------------------- */
/* 4-D permute of a (N, d0,d1,d2,d3) tensor: out dim i = in dim order[i].  Replaces
 * TransformPlugin::enqueue -> cudnnTransformTensor (lib/transform_plugin.cpp:94-108). */
int rt_permute4d(const void* x, void* y, int batch, int d0, int d1, int d2, int d3, const int order[4],
                 int dtype, rtStream stream);
/* Format conversion at a plugin boundary -- the "reformat" TensorRT inserts between its fp32 tensors and an IPluginExt that
 * asked for kHALF (reference lib/elu_plugin.cpp:45-53, lib/cost_volume_plugin.cpp:60-66; tests_main.cpp:301-321, 988-1026).
 * Kinds: 0 = fp32 NCHW, 1 = fp16 NCHW, 2 = fp16 NC2HW2 (channel pairs of a pixel in one 4-byte slot, odd C zero padded).
 * x / y: (batch, C, inner) with inner = the product of the remaining dims. */
int rt_convert_format(const void* x, void* y, int batch, int C, int64_t inner, int src_kind, int dst_kind, rtStream stream);

/* (N,D,inner) -> (N,D+pad_end,inner): copy + zero tail.  PaddingPlugin::enqueue (lib/padding_plugin.cpp:79-94). */
int rt_pad_d(const void* x, void* y, int batch, int D, int64_t inner, int pad_end, int dtype, rtStream stream);
/* (N,D,inner) -> (N,end-start,inner).  SlicePlugin::enqueue (lib/slice_plugin.cpp:80-92). */
int rt_slice_d(const void* x, void* y, int batch, int D, int64_t inner, int start, int end, int dtype,
               rtStream stream);
/* Copy `C` channels of x (N,C,inner) into channels [c_off, c_off+C) of y (N,Ctot,inner):
 * TensorRT addConcatenation, sample_app/resnet18_2D_513x257_net.cpp:612-615. */
int rt_concat_channels(const void* x, void* y, int batch, int C, int Ctot, int c_off, int64_t inner, int dtype,
                       rtStream stream);

/* ---- image front-end / back-end of the sample application ----------------------------------- */
/* u8 BGR HWC image(s) (N, src_h, src_w, 3) -> float RGB CHW (N, 3, dst_h, dst_w) in [0,1]: convertTo(CV_32F),
 * cv::resize(INTER_AREA) (down-scaling or same size), BGR -> RGB, HWC -> CHW, / 255 of readImgFile
 * (sample_app/main.cpp:83-98; stereo_dnn_ros_node.cpp:42-103), on the device. */
int rt_preprocess_bgr8(const void* src_u8, int src_h, int src_w, void* dst_f32, int dst_h, int dst_w, int batch,
                       rtStream stream);
/* Colour encodings of sensor_msgs/Image the ROS node accepts (stereo_dnn_ros_node.cpp:112-119), plus rgba8. */
enum { RT_ENC_BGR8 = 0, RT_ENC_RGB8 = 1, RT_ENC_BGRA8 = 2, RT_ENC_RGBA8 = 3 };
/* Both frames of a stereo pair as the camera delivers them -> float RGB CHW (N, 3, dst_h, dst_w) in [0,1] each: the per-frame
 * path of the ROS node's computeOutputs / preprocessImage (stereo_dnn_ros_node.cpp:42-58, 60-77: cvtColor(BGR2RGB / BGRA2RGB),
 * convertTo(CV_32F), cv::resize(INTER_AREA), / 255, HWC -> CHW) in one launch for the whole pair batch.  Frame n of a side
 * starts at `base + n * src_h * src_step` bytes, row y at `src_step * y` (the sensor_msgs/Image `step`; >= src_w * 3 or * 4).
 * Alpha is dropped.  Bit-identical to rt_preprocess_bgr8 on the dense BGR form of the same pixels; the same limits
 * (down-scaling or same size, factors <= 6, else RT_E_UNSUPPORTED). */
int rt_preprocess_frames_u8(const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step, int encoding,
                            void* left_f32, void* right_f32, int dst_h, int dst_w, int batch, rtStream stream);
/* out = disp * scale, fp32, in place allowed: the ROS node's `output *= w` (stereo_dnn_ros_node.cpp:81) and the sample app's
 * `img_f *= w` (sample_app/main.cpp:325-327) on the device. */
int rt_disparity_scale(const void* disp_f32, void* out_f32, int64_t n, float scale, rtStream stream);
/* disparity map -> 16-bit KITTI encoding: saturate_cast<ushort>(round(disp * scale)), scale = 256 (x width for the
 * normalised output of ResNet-18 2D), sample_app/main.cpp:324-330. */
int rt_disparity_to_u16(const void* disp_f32, void* out_u16, int64_t n, float scale, rtStream stream);

/* ---- left-right consistency check (no counterpart in the reference) --------------------------- */
/* A left-referenced network gives the right view's disparity when it is fed the mirrored right image as "left" and the mirrored left
 * image as "right": its output, mirrored back, is referenced to the right view.  The two calls below are the front and the back end of
 * that second pass as the second half of one batch (rt_stereo_net.h: rt_net_execute_frames_lr ties them to an engine).
 *
 * As rt_preprocess_frames_u8 for images [0, batch) of left_dst / right_dst, which here hold 2 * batch images each; bit-identical to it.
 * Images [batch, 2 * batch) are the mirrored, swapped pair:  left_dst[batch + n] (c, y, x) = right_dst[n](c, y, W-1-x)
 *                                                             right_dst[batch + n](c, y, x) = left_dst[n] (c, y, W-1-x)
 * (the mirror of the pre-processed planes, not the planes of the mirrored frame: each value is computed once and stored twice).
 * Same limits and refusals as rt_preprocess_frames_u8, found before anything is written. */
int rt_preprocess_frames_u8_lr(const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step, int encoding,
                               void* left_dst, void* right_dst, int dst_h, int dst_w, int batch, rtStream stream);
/* Forms of a disparity output (rt_lr_consistency; rt_stereo_net.h: rt_net_execute_frames), for a model whose pixel scale is `scale`:
 *   RT_DISP_NET         fp32, the network's value        RT_DISP_PIXELS_F32  fp32, value * scale
 *   RT_DISP_KITTI_U16   uint16, rt_disparity_to_u16(value, 256 * scale) */
enum { RT_DISP_NET = 0, RT_DISP_PIXELS_F32 = 1, RT_DISP_KITTI_U16 = 2 };
/* The check, the mask and the output encoding in one launch.
 * net_disp:    (2 * batch, 1, H, W) fp32 as the engine wrote it for the batch of rt_preprocess_frames_u8_lr
 * out:         (batch, 1, H, W) in out_kind, invalid pixels = 0
 * mask_u8:     (batch, 1, H, W) uint8, 255 = consistent, 0 = not; may be NULL
 * right_out:   (batch, 1, H, W) the right view's disparity, un-mirrored and unmasked, in out_kind; may be NULL
 * valid_count: device array of `batch` uint64, number of consistent pixels per image; may be NULL
 * All in fp32, every operation rounded on its own (nothing is contracted into an FMA):
 *   dL(x) = net_disp[n, 0, y, x] * scale                     left view, pixels
 *   dR(x) = net_disp[batch + n, 0, y, W-1-x] * scale         right view, pixels, un-mirrored
 *   xr    = rintf((float)x - dL(x))                          nearest column in the right view, ties to even
 *   valid = 0 <= xr <= W-1  and  fabsf(dL(x) - dR(xr)) <= max_diff_px        (a NaN anywhere: not valid)
 * `scale` is the model's pixel scale (width for ResNet-18 2D, 1 for the 3-D models) for every out_kind: the check is always done in
 * pixels.  A valid pixel of RT_DISP_KITTI_U16 that encodes to 0 is raised to 1 (the KITTI devkit's rule), so that 0 always and only
 * means "no value" there; for the fp32 kinds, where 0 can be a value, the mask is the authority.  right_out is not masked and not raised.
 * The outputs must not overlap net_disp.  max_diff_px < 0 or NaN, an unknown kind, batch / H / W < 1, a null net_disp or out: error,
 * nothing written. */
int rt_lr_consistency(const void* net_disp, int batch, int H, int W, float scale, float max_diff_px, void* out, int out_kind,
                      void* mask_u8, void* right_out, void* valid_count, rtStream stream);

/* ---- speckle filter (no counterpart in the reference; stereo_image_proc's speckle_size / speckle_range, cv::filterSpeckles) ------------ */
/* Removes small connected blobs of a disparity map: what the left-right check leaves inside its holes and along depth edges, and what
 * rt_disparity_to_points would turn into clusters of points floating in space.  Its place is network geometry, between rt_lr_consistency
 * (or rt_disparity_scale) and rt_disparity_to_frame / rt_disparity_to_points, whose "do not mix with invalid taps" rule then sees the
 * removed pixels.
 * disp_px:  (batch,1,H,W) fp32      mask_u8: (batch,1,H,W) the 255 / 0 mask of rt_lr_consistency, or NULL
 * A pixel is LIVE iff (mask_u8 == NULL || mask != 0) && d == d: a NaN is never live; an infinity is live but adjacent to nothing.
 * Two live pixels of the same image are ADJACENT iff they are 4-neighbours (left / right in a row, up / down in a column) and
 *   fabsf(d(p) - d(q)) <= max_diff_px     in fp32, the difference and the comparison each rounded on its own
 * (-0.f and 0.f are adjacent at max_diff_px = 0).  Nothing wraps from the end of a row to the next row, nothing joins image n to image
 * n + 1.  COMPONENTS are the classes of the transitive closure of adjacency -- cv::filterSpeckles' neighbour-to-neighbour region growing:
 * a ramp of small steps is one component whatever its end-to-end range.  A component is a SPECKLE iff it has <= max_size pixels
 * (OpenCV's rule: larger blobs are not affected).  keep(p) = live and not in a speckle, and
 *   out[p]         = keep ? disp_px[p] : 0.f      (the bits are copied, nothing is recomputed)
 *   out_mask_u8[p] = keep ? 255 : 0               uint8, may be NULL
 *   valid_count[n] = kept pixels of image n       `batch` uint64 on the device, zeroed by the entry, may be NULL
 * max_size == 0 is legal and removes nothing: mask = live, value or 0.  out == disp_px and out_mask_u8 == mask_u8 are legal (in place,
 * bit-identical to the out-of-place call); no other overlap is.  The result is a pure function of the inputs -- which pixels go depends
 * only on integer component sizes -- so every run is bit-identical, in whatever order the device ran the work.
 * `workspace`: device memory of rt_speckle_workspace_bytes(batch, H, W) bytes (one label and one size word per pixel), 4-byte aligned,
 * private to the stream until the launches have run: four of them (tiles, tile borders, sizes, apply), one when max_size == 0.
 * Errors, found before anything is written: a null disp_px or out; batch, H or W < 1; H * W >= 2^31 or batch > 32767; max_size < 0;
 * max_diff_px negative, NaN or infinite; a missing or short workspace.  rt_speckle_workspace_bytes returns 0 for sizes the op refuses. */
size_t rt_speckle_workspace_bytes(int batch, int H, int W);
int rt_disparity_speckle(const void* disp_px, const void* mask_u8, int batch, int H, int W, int max_size, float max_diff_px,
                         void* out, void* out_mask_u8, void* valid_count, void* workspace, size_t workspace_bytes, rtStream stream);

/* ---- frames of any size in, disparity at the frame's size out ------------------------------------------------------------------ */
/* The whole of cv::resize(INTER_AREA) on the fp32 image as the ROS node calls it for whatever the camera sends
 * (stereo_dnn_ros_node.cpp:42-58), for both frames of a pair batch in one launch.  Arguments as rt_preprocess_frames_u8.
 *   dst_h <= src_h and dst_w <= src_w: the box filter; bit-identical to rt_preprocess_frames_u8 (the same code).
 *   otherwise (either axis grows): OpenCV does not mix filters per axis -- "true area interpolation is only implemented for
 *   scale_x >= 1 && scale_y >= 1; in other cases it is emulated using some variant of bilinear" -- so BOTH axes use the two-tap set-up
 *   of its area_mode branch, the shrinking one included.  Per axis, source size n, destination size m, destination index d, positions
 *   in double, the weight cast to fp32:
 *       inv = (double)m / n;   scale = 1.0 / inv
 *       s   = (int)floor(d * scale)
 *       f   = (float)((d + 1) - (s + 1) * inv);   f = f <= 0 ? 0.f : f - floorf(f)
 *       if (s >= n - 1) { s = n - 1; f = 0.f; }
 *       taps: source s with weight 1.f - f, source min(s + 1, n - 1) with weight f
 *   (s + 1) * inv is rounded before the subtraction: nothing in the tap set-up is contracted into an FMA.  Value, per channel, fp32, x
 *   first, every product and sum rounded on its own:  row_j = S[y_j][x0] * a0 + S[y_j][x1] * a1  for the two rows,
 *   v = row_0 * b0 + row_1 * b1,  then colour order, / 255.f and planes exactly as rt_preprocess_frames_u8.  A pure integer
 *   magnification thereby replicates pixels (INTER_AREA's known behaviour); the same size is a copy.
 * mirror_twin != 0: left_dst / right_dst hold 2 * batch images and images [batch, 2 batch) are the mirrored, swapped pair as
 * rt_preprocess_frames_u8_lr defines it; in the box case bit-identical to rt_preprocess_frames_u8_lr.
 * Limits: every axis factor src / dst within [1/6, 6], else RT_E_UNSUPPORTED; a short src_step, an unknown encoding, null pointers,
 * batch < 1: error.  All found before anything is written. */
int rt_preprocess_frames_u8_cv(const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step, int encoding,
                               void* left_dst, void* right_dst, int dst_h, int dst_w, int batch, int mirror_twin, rtStream stream);
/* The way back: disparity in the network's geometry -> disparity in the frame's geometry, in the frame's pixels, one launch.
 * disp_px:  (batch,1,H,W) fp32, pixels of the network's geometry (what RT_DISP_PIXELS_F32 holds)
 * mask_u8:  (batch,1,H,W) the 255 / 0 mask of rt_lr_consistency, or NULL
 * out:      (batch,1,out_h,out_w) in out_kind: RT_DISP_PIXELS_F32 or RT_DISP_KITTI_U16
 * out_mask_u8: (batch,1,out_h,out_w) uint8 or NULL;  valid_count: `batch` uint64 on the device or NULL, zeroed by the entry;
 *           both only with mask_u8
 * All fp32, nothing contracted.  Per axis (n source, m destination, index d), half-pixel centres (bilinear, align_corners = false):
 *       sc = (float)n / (float)m;   p = ((float)d + 0.5f) * sc - 0.5f;   p = p < 0 ? 0 : p
 *       i0 = min((int)floorf(p), n - 1);   i1 = min(i0 + 1, n - 1);   w1 = p - (float)i0;   w0 = 1.f - w1
 *   top = D[y0][x0] * a0 + D[y0][x1] * a1,  bot likewise on y1,  v = (top * b0 + bot * b1) * r  with r = (float)out_w / (float)W
 *   (disparities scale with the width ratio only).  RT_DISP_KITTI_U16: rintf(v * 256.f) saturated to [0, 65535] as rt_disparity_to_u16;
 *   a NaN encodes to 0.
 * With mask_u8: the nearest tap is x1 if a1 > 0.5f else x0, the same in y.  If all four taps are valid, v as above; otherwise
 * v = D[nearest] * r (nothing is mixed with the zeros the check wrote).  The frame pixel is valid iff its nearest tap is; an invalid
 * pixel is 0 in out and in out_mask_u8; a valid RT_DISP_KITTI_U16 value that encodes to 0 is raised to 1 (as rt_lr_consistency).
 * out_h == H && out_w == W is legal: a copy / an encoding.  Factors within [1/6, 6] per axis, else RT_E_UNSUPPORTED; another kind, null
 * disp_px / out, sizes < 1, out_mask_u8 / valid_count without mask_u8: error.  All found before anything is written. */
int rt_disparity_to_frame(const void* disp_px, const void* mask_u8, int batch, int H, int W, void* out, int out_kind, int out_h,
                          int out_w, void* out_mask_u8, void* valid_count, rtStream stream);

/* ---- depth and a point cloud out (no counterpart in the reference; what stereo_image_proc publishes behind such a node) --------- */
/* A rectified pair in the geometry of the OUTPUT (out_h x out_w), from sensor_msgs/CameraInfo: P of the left camera gives
 * fx = P[0], fy = P[5], cx = P[2], cy = P[6] (cx, cy in pixel-index units: pixel u has its centre at u); P of the right camera gives
 * baseline = -P_right[3] / P_right[0] in metres (> 0) and doffs = P_right[2] - P_left[2] in pixels (0 for a ZED or a
 * stereoRectify with CALIB_ZERO_DISPARITY). */
typedef struct rtStereoCamera {
    float fx, fy, cx, cy;
    float baseline;
    float doffs;
} rtStereoCamera;
/* REP 118 depth images: 32FC1 metres, NaN (0x7fc00000) = no value; 16UC1 millimetres, 0 = no value */
enum { RT_DEPTH_M_F32 = 0, RT_DEPTH_MM_U16 = 1 };
/* rt_disparity_to_frame followed, without a trip through memory, by the reprojection.  disp_px, mask_u8, H, W, out_h, out_w, disp_out /
 * disp_kind, out_mask_u8 and valid_count are rt_disparity_to_frame's arguments (disp_out its `out`): those three outputs are bit-identical
 * to what it writes and follow its validity `valid0` (true without a mask), not the depth range.  Every output may be NULL, one at
 * least must be given.  All fp32, nothing contracted, IEEE divisions.  For output pixel (row r, column u) with resampled disparity v:
 *   den = v + doffs;  ok = valid0 && den > 0 && den finite;  Z = fB / den  with fB = fx * baseline (formed once, in fp32);
 *   ok = ok && Z >= min_depth && Z <= max_depth;   X = (((float)u - cx) / fx) * Z;   Y = (((float)r - cy) / fy) * Z
 *   depth          (batch,1,out_h,out_w): RT_DEPTH_M_F32  ok ? Z : NaN;   RT_DEPTH_MM_U16  ok ? max(1, sat_u16(rintf(Z * 1000.f))) : 0
 *   points         (batch,out_h,out_w) records of 16 bytes {float x, y, z; uint32 rgb = R << 16 | G << 8 | B} (PCL's PointXYZRGB packing:
 *                  PointCloud2 fields x / y / z / rgb at offsets 0 / 4 / 8 / 12, point_step 16); x = y = z = NaN where not ok, the colour
 *                  is written for every pixel (is_dense = false)
 *   points_compact the ok records of image n in row-major order from byte n * out_h * out_w * 16 on (bytes behind the last one are not
 *                  touched), and count[n] (`batch` uint64 on the device) their number; count alone is legal.  The order is deterministic.
 *   colour         the left frames, out_h x out_w pixels in `encoding` (RT_ENC_*), rows color_step bytes apart, addressed as
 *                  rt_preprocess_frames_u8 addresses frames; alpha is dropped; color_u8 == NULL: rgb = 0
 * A compact cloud or a count needs `workspace`, device memory of rt_points_workspace_bytes(batch, out_h, out_w) bytes, and one more
 * launch than the single one everything else takes.  A cloud must start on a 16-byte boundary.
 * Errors, found before anything is written: null disp_px or cam; no output; sizes < 1; fx, fy or baseline not finite or not > 0; cx, cy
 * or doffs not finite; min_depth NaN or < 0; max_depth NaN or < min_depth (+inf is legal); an unknown kind of a given output; with a
 * colour an unknown encoding or a color_step shorter than a row; points_compact without count; out_mask_u8 / valid_count without mask_u8;
 * a missing or short workspace; a cloud off a 16-byte boundary.  Factors outside [1/6, 6] per axis: RT_E_UNSUPPORTED. */
size_t rt_points_workspace_bytes(int batch, int out_h, int out_w);
int rt_disparity_to_points(const void* disp_px, const void* mask_u8, int batch, int H, int W, int out_h, int out_w,
                           const rtStereoCamera* cam, float min_depth, float max_depth, const void* color_u8, int64_t color_step,
                           int encoding, void* disp_out, int disp_kind, void* out_mask_u8, void* valid_count, void* depth, int depth_kind,
                           void* points, void* points_compact, void* count, void* workspace, size_t workspace_bytes, rtStream stream);

/* ---- the cloud on a voxel grid (no counterpart in the reference; pcl::VoxelGrid, the node behind stereo_image_proc/point_cloud2) --------- */
/* A box of dims[0] x dims[1] x dims[2] cells of leaf[0] x leaf[1] x leaf[2] metres whose corner is `origin`, axes x, y, z of the camera
 * frame the cloud is in. */
typedef struct rtVoxelGrid { float origin[3]; float leaf[3]; int dims[3]; } rtVoxelGrid;   /* x, y, z; camera frame, metres */
/* One record per occupied cell of the grid: the centroid of the cell's points and their mean colour.  What a planner, an octomap or a
 * collision checker takes instead of one point per pixel.
 * points:  (batch, capacity) records of 16 bytes {float x, y, z; uint32 rgb} as rt_disparity_to_points writes them; image n starts at record
 *          n * capacity.  count == NULL: all `capacity` records of an image are read (the organised cloud, whose invalid pixels are NaN).
 *          Otherwise count is `batch` uint64 on the device and only the first min(count[n], capacity) records of image n are read
 *          (points_compact with its count).
 * CELL of a point, per axis a, all fp32, every operation rounded on its own, the division IEEE, nothing contracted:
 *   t_a = (p_a - origin_a) / leaf_a
 *   the point is IN THE GRID iff for all three axes  t_a >= 0.f && t_a < (float)dims_a   (a NaN fails: invalid pixels drop out; so does
 *   an infinity)
 *   i_a = (int)floorf(t_a);   cell = (i_z * dims_y + i_y) * dims_x + i_x
 *   f_a = t_a - floorf(t_a)   (exact);   q_a = (uint32)(f_a * 65536.f)   (truncated; in [0, 65535])
 * Per VOXEL -- a cell with at least one point of image n -- integer sums, so their order does not matter:
 *   N = number of points;   S_a = sum of q_a;   R, G, B = sums of the colour bytes (rgb >> 16 & 255, rgb >> 8 & 255, rgb & 255)
 * A voxel is EMITTED iff N >= min_points, as the record
 *   g_a = ((double)S_a / (double)N + 0.5) / 65536.0                                  in double
 *   c_a = (origin_a + (float)i_a * leaf_a) + (float)g_a * leaf_a                     in fp32, each operation rounded on its own
 *   rgb = r << 16 | g << 8 | b  with  r = (R + N / 2) / N  in integer arithmetic, g and b likewise
 * (the centroid from 16-bit offsets inside the cell: it differs from the mean of the floats by less than leaf_a / 131072 plus fp32
 * rounding).
 * voxels:  the emitted voxels of image n IN ASCENDING cell from byte n * out_capacity * 16 on, {float c_x, c_y, c_z; uint32 rgb}; at most
 *          out_capacity records are written, the first ones in that order; bytes behind the last record are not touched.
 * out_count:    `batch` uint64 on the device, zeroed by the entry, required: the number of emitted voxels of image n whether or not they
 *               fitted (out_count[n] > out_capacity: the cloud was truncated).
 * out_cell_u32, out_n_u32: optional, laid out like voxels with 4 bytes per record: `cell` and N of each written record (an occupancy
 *               grid's index; a weight).
 * The result is a pure function of the SET of points of each image: permuting an image's records changes no bit, the compact and the
 * organised cloud of one rt_disparity_to_points call give the same bytes, and every run is bit-identical, in whatever order the device ran
 * the work.
 * `workspace`: device memory of rt_voxel_workspace_bytes(batch, capacity, grid) bytes, 8-byte aligned, private to the stream until the
 * launches have run; nothing depends on what it held.  Per image it is one bit and one prefix word per 32 cells, 44 bytes per slot with
 * min(capacity, cells) slots, and the scans' block sums: a 2^27-cell grid costs 32 MiB and a memset of 16 MiB, whatever the cloud's size.
 * Launches: mark, two for the scan, zero, accumulate, emit; two more with min_points > 1.
 * Errors, found before anything is written: a null points, grid, voxels or out_count; batch < 1 or > 32767; capacity or out_capacity
 * outside [1, 2^23] (2^23 keeps the colour sums inside 32 bits); a dims entry outside [1, 4096] or more than 2^27 cells; a leaf that is
 * not finite and > 0; an origin that is not finite; min_points < 1; points or voxels off a 16-byte boundary (the counts: 8, out_cell_u32
 * and out_n_u32: 4); a missing, short or misaligned workspace; any overlap of an output or the workspace with an input or with one
 * another.  rt_voxel_workspace_bytes returns 0 for a batch, a capacity or a grid the op refuses. */
size_t rt_voxel_workspace_bytes(int batch, int capacity, const rtVoxelGrid* grid);          /* 0 for what the op refuses */
int rt_points_voxel_grid(const void* points, const void* count, int batch, int capacity, const rtVoxelGrid* grid, int min_points,
                         void* voxels, int out_capacity, void* out_count, void* out_cell_u32, void* out_n_u32,
                         void* workspace, size_t workspace_bytes, rtStream stream);

/* ---- raw frames in: rectification (image_proc's stage in front of stereo_image_proc; the reference node subscribes to image_rect_color) -- */
/* One camera of the rig, from its sensor_msgs/CameraInfo (all float64 there). */
typedef struct rtRectifyCamera {
    double fx, fy, cx, cy;   /* K[0], K[4], K[2], K[5]; skew K[1] is ignored, as OpenCV's initUndistortRectifyMap ignores it */
    double d[8];             /* k1 k2 p1 p2 k3 k4 k5 k6: plumb_bob = the first five, rest 0; rational_polynomial = all eight */
    double iR[9];            /* inverse of P[:, :3] * R, row-major */
} rtRectifyCamera;
/* Host only: K, R row-major 3x3, P row-major 3x4, D the n_d first coefficients in the order of d (0, 4, 5 or 8 of them, the rest 0).  iR is a
 * 3x3 inverse in double.  Another n_d, a non-finite entry, a singular P[:, :3] * R: error, *out untouched. */
int rt_rectify_camera_from_info(const double K[9], const double* D, int n_d, const double R[9], const double P[12], rtRectifyCamera* out);
/* Raw frames -> rectified frames, both frames of a pair batch in one launch.  Frames are addressed exactly as rt_preprocess_frames_u8
 * addresses them (RT_ENC_*, rows `step` bytes apart, frame n at n * h * step); the output keeps the input's encoding and bytes per pixel;
 * for the 4-byte encodings alpha is interpolated like a colour channel (as cv::remap treats a 4-channel Mat); bytes between a row's last
 * pixel and dst_step are not touched.  One camera pair serves the whole batch.  Source and destination must not overlap.
 * The map: cv::initUndistortRectifyMap's model evaluated per pixel.  For destination row v and column u, taken as doubles, everything in
 * double, every operation rounded on its own (nothing contracted, IEEE division), in exactly this order:
 *   X = (iR[0]*u + iR[1]*v) + iR[2]     Y = (iR[3]*u + iR[4]*v) + iR[5]     W = (iR[6]*u + iR[7]*v) + iR[8]
 *   x = X / W,  y = Y / W,  x2 = x*x,  y2 = y*y,  r2 = x2 + y2,  xy2 = (2*x)*y
 *   kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
 *   xd = (x*kr + p1*xy2) + p2*(r2 + 2*x2)          yd = (y*kr + p1*(r2 + 2*y2)) + p2*xy2
 *   mx = (float)(fx*xd + cx)                       my = (float)(fy*yd + cy)
 * (OpenCV accumulates X, Y, W along the row and so differs in the last bits; this statement is the target, not OpenCV's bits.)
 * The sampler: cv::remap(INTER_LINEAR, BORDER_CONSTANT, 0) in fp32, every operation rounded on its own.  A pixel is inside iff
 * mx > -1 && mx < src_w && my > -1 && my < src_h, compared in fp32 before anything is made an integer (a NaN fails it); a pixel that is
 * not inside has every byte 0.  Otherwise x0 = floorf(mx), a = mx - x0, y0 = floorf(my), b = my - y0, a tap outside the source image has
 * the value 0, and per channel
 *   top = S00*(1-a) + S01*a,   bot = S10*(1-a) + S11*a,   v = top*(1-b) + bot*b,   byte = rintf(v)
 * (fp32 weights, where cv::remap rounds them to 5 fractional bits.)
 * rt_rectify_maps writes (mx, my) of one camera as two (dst_h, dst_w) fp32 planes, the CV_32FC1 pair of initUndistortRectifyMap;
 * rt_remap_frames_u8 is the sampler on maps of the caller (shared by the batch; any model, a fisheye one included).
 * rt_rectify_frames_u8 is by definition rt_rectify_maps for each camera followed by rt_remap_frames_u8, bit for bit; it forms the
 * positions in registers and never writes a map.
 * Errors, found before anything is written: null pointers; an unknown encoding; a step (source or destination) shorter than a row; a
 * size < 1; a non-finite field of a camera; left_dst == left_u8 or right_dst == right_u8. */
int rt_rectify_frames_u8(const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step, int encoding,
                         const rtRectifyCamera* cam_left, const rtRectifyCamera* cam_right,
                         void* left_dst, void* right_dst, int dst_h, int dst_w, int64_t dst_step, int batch, rtStream stream);
int rt_rectify_maps(const rtRectifyCamera* cam, int dst_h, int dst_w, void* map_x_f32, void* map_y_f32, rtStream stream);
int rt_remap_frames_u8(const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step, int encoding,
                       const void* map_x_left, const void* map_y_left, const void* map_x_right, const void* map_y_right,
                       void* left_dst, void* right_dst, int dst_h, int dst_w, int64_t dst_step, int batch, rtStream stream);

/* ---- what the camera really sends: mono, Bayer and YUV 4:2:2 (image_proc's debayer and cv_bridge's colour conversion, on the device) ---- */
/* Wire encodings of sensor_msgs/Image, a set of their own beside RT_ENC_*: only rt_decode_frames_u8 (and rtDecodeCall, rt_stereo_net.h) takes
 * them, every other call goes on refusing them.  Bytes per pixel: 1, 2, 1, 1, 1, 1, 2, 2.  The Bayer names are those of
 * sensor_msgs/image_encodings.h: the four letters are the top-left 2 x 2 of the mosaic, row-major -- rggb: row 0 is R G, row 1 is G B;
 * bggr: B G / G R;  gbrg: G B / R G;  grbg: G R / B G.  (OpenCV's COLOR_Bayer* constants are named after another corner: go by the
 * pattern, not by those names.) */
enum { RT_WIRE_MONO8 = 16, RT_WIRE_MONO16 = 17,
       RT_WIRE_BAYER_RGGB8 = 18, RT_WIRE_BAYER_BGGR8 = 19, RT_WIRE_BAYER_GBRG8 = 20, RT_WIRE_BAYER_GRBG8 = 21,
       RT_WIRE_YUV422 = 22 /* UYVY */, RT_WIRE_YUV422_YUY2 = 23 /* YUYV */ };
/* Wire frames -> colour frames, both frames of a pair batch in one launch.  Frames are addressed exactly as rt_preprocess_frames_u8
 * addresses them (rows `step` bytes apart, frame n at n * h * step; any step, any base alignment); the output is h x w pixels in
 * dst_encoding (RT_ENC_*), alpha = 255 for the 4-byte encodings; bytes between a row's last pixel and dst_step are not touched.
 * Integer arithmetic throughout, >> on a negative value is an arithmetic shift (floor).
 *   MONO8    R = G = B = v.
 *   MONO16   little-endian, v16 = b[2x] | b[2x+1] << 8;  R = G = B = min(255, (v16 + 127 + ((v16 >> 8) & 1)) >> 8): rint(v16 / 256) with ties
 *            to even, saturated -- cv_bridge's 16 -> 8 bit conversion, convertTo(CV_8U, 1 / 256.).  is_bigendian images are not supported:
 *            swap the bytes first.
 *   BAYER_*8 bilinear demosaicing.  m(y, x) is the mosaic, extended by reflection about the edge sample (BORDER_REFLECT_101): index
 *            i < 0 is -i, i > n - 1 is 2 (n - 1) - i.  Reflection keeps the colour phase, so one formula serves every pixel.  The site's
 *            colour is pattern[y & 1][x & 1].  At an R or B site of colour C, with C' the other one of R and B:
 *              C = m(y,x);   G  = (m(y,x-1) + m(y,x+1) + m(y-1,x) + m(y+1,x) + 2) >> 2;
 *              C' = (m(y-1,x-1) + m(y-1,x+1) + m(y+1,x-1) + m(y+1,x+1) + 2) >> 2
 *            At a G site: G = m(y,x); the colour of the horizontal neighbours, pattern[y & 1][(x & 1) ^ 1], is (m(y,x-1) + m(y,x+1) + 1) >> 1
 *            and the colour of the vertical neighbours is (m(y-1,x) + m(y+1,x) + 1) >> 1.  Needs h >= 2 and w >= 2; odd sizes are legal.
 *            In the interior this is the arithmetic of OpenCV's bilinear demosaicing (image_proc's default for 8 bit).  At the one-pixel
 *            frame OpenCV replicates the neighbouring OUTPUT pixel; the reflection here is a deliberate difference.
 *   YUV422 / YUV422_YUY2   the 4 bytes of a pixel pair are U Y0 V Y1 (YUV422) or Y0 U Y1 V (YUV422_YUY2); w must be even; both pixels of a
 *            pair share U and V.  OpenCV's integer BT.601 limited-range conversion (cvtColor(COLOR_YUV2BGR_UYVY / _YUY2)), which fits 32-bit
 *            signed integers:  CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527,  y = max(0, Y - 16) * CY,
 *              R = clamp((y + (1 << 19) + CVR * (V - 128)) >> 20, 0, 255)
 *              G = clamp((y + (1 << 19) + CVG * (V - 128) + CUG * (U - 128)) >> 20, 0, 255)
 *              B = clamp((y + (1 << 19) + CUB * (U - 128)) >> 20, 0, 255)
 * This statement is the target, held by the properties tests/test_decode.py lists; it was not compared with OpenCV's output.
 * Errors, found before anything is written: a null pointer; a wire_encoding outside RT_WIRE_* (RT_ENC_* values included); a dst_encoding
 * outside RT_ENC_*; h, w or batch < 1, h > 4 * 65535, w > 2^24, batch > 32767; a Bayer frame with h < 2 or w < 2; an odd w for the two YUV
 * encodings; a wire_step shorter than w wire pixels; a dst_step shorter than w output pixels; a destination that is a source (or the other
 * destination). */
int rt_decode_frames_u8(const void* left_wire, const void* right_wire, int h, int w, int64_t wire_step, int wire_encoding,
                        void* left_u8, void* right_u8, int64_t dst_step, int dst_encoding /* RT_ENC_* */, int batch, rtStream stream);

/* ---- the viz node's debug panel (ros/packages/stereo_dnn_ros_viz/src/stereo_dnn_ros_viz_node.cpp) ---------------------------- */
/* KITTI colour scheme of the viz node's dispToColor (:49-79): disp_px (n,1,H,W) fp32 pixels -> rgb8, rows dst_step >= 3W bytes apart,
 * images H * dst_step bytes apart; bytes between 3W and dst_step are not touched.  With the reference's fp32 tables
 *   weights = {8.77192974, 5.40540552, 8.77192974, 5.74712658, 8.77192974, 5.40540552, 8.77192974, 0}
 *   cumsum  = {0, 0.114, 0.299, 0.413, 0.587, 0.70100003, 0.88600004, 1},   w_map[i] = (i>>1 & 1, i>>2 & 1, i & 1) as (R, G, B):
 *   cur   = d / max_disp                                   fp32 division
 *   index = the largest i in 0..7 with i == 0 or cur > cumsum[i]            (NaN: 0)
 *   w     = (float)(1.0 - (double)((cur - cumsum[index]) * weights[index]))  subtraction and product in fp32, each rounded on its own
 *   c     = trunc(clamp((w * w_map[index][c] + (1 - w) * w_map[index+1][c]) * 255, 0, 255))   in double; a map entry of 0 contributes 0
 * Where the reference is undefined: cur > 1 gives index 7 and w = 1 (also for an infinite cur, where inf * 0 would be NaN), and the
 * row w_map[8] the reference reads past its table counts as 0: white.  A negative cur makes 1 - w negative, which the reference casts
 * to uint8_t: here the clamp gives 0.  NaN: black.  max_disp must be a finite number > 0 (the node hard-codes 96). */
int rt_disparity_to_color(const void* disp_px, int batch, int H, int W, float max_disp, void* dst_rgb8, int64_t dst_step, rtStream stream);
/* The viz node's whole panel (computeOutput, :81-130) in one launch: per image a (2H) x (2W) rgb8 picture, rows dst_step >= 6W bytes
 * apart, images 2H * dst_step bytes apart, padding bytes not touched:
 *   top-left     the left frame, top-right the right frame: RT_ENC_* frames of src_h x src_w pixels, rows src_step bytes apart, as
 *                rt_preprocess_frames_u8 takes them, area-resized to H x W, in R,G,B order: each channel is rintf (ties to even) of the
 *                fp32 area average rt_preprocess_frames_u8 forms before its / 255, clamped to [0, 255]; alpha is dropped
 *   bottom-left  disparity as grey: rintf(d * s) clamped to [0, 255], s = 255.f / max_disp in fp32, NaN -> 0.  (The node's
 *                `output *= 255.0 / 96` goes through OpenCV's scaled conversion, whose rounding of the factor depends on the version.)
 *   bottom-right disparity in the KITTI colour scheme: exactly the bytes of rt_disparity_to_color
 * A disparity of 0 -- what rt_net_execute_frames_lr writes at inconsistent pixels -- is black in both bottom panels.
 * Limits and refusals as rt_preprocess_frames_u8 (down-scaling or same size, factors <= 6, else RT_E_UNSUPPORTED; a short src_step,
 * an unknown encoding, null pointers, batch < 1), plus dst_step < 6W and a max_disp that is not a finite number > 0; all found before
 * anything is written. */
int rt_viz_mosaic_u8(const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step, int encoding,
                     const void* disp_px, int H, int W, float max_disp, void* dst_rgb8, int64_t dst_step, int batch, rtStream stream);

/* ---- convolutions (MFMA implicit GEMM) ----------------------------------------------------- */
/* A plan owns the device copy of the (re-packed) weights, bias and gather tables of one layer,
 * like Conv3DPlugin::configure owns kernel_weights_d_ (lib/conv3d_plugin.cpp:122-133). */
typedef struct rtConvPlan rtConvPlan;

typedef struct rtConv2dDesc {
    int Cin, Cout;          /* channels                                                          */
    int Hin, Win;           /* input plane                                                       */
    int KH, KW;             /* 3x3 or 5x5                                                        */
    int stride;             /* 1 or 2 (same in H and W)                                          */
    int pad_h, pad_w;       /* symmetric zero padding (TRT setPadding)                           */
    int act;                /* RT_ACT_* fused after bias (+ residual)                            */
    int has_residual;       /* enqueue takes a residual tensor shaped like the output            */
    int dtype;              /* RT_F32 | RT_F16: storage type of activations AND weights          */
    int flags;              /* RT_CONV_* option bits, 0 = defaults                               */
} rtConv2dDesc;

/* rtConv2dDesc::flags / rtConv3dDesc::flags.  RT_CONV_EXACT_FP32: keep the convolution on the fp32 fmaf-chain kernels (fp32 MFMA /
 * Winograd F(2x2,3x3)) instead of the default 3-term fp16 split on the fp16 matrix pipe (22-bit operands, fp32 accumulation; domain
 * |x| < 65504, see rt_check_range).  IBuilder::setExactFp32Mode / rtNetOptions::flags set it for a whole engine. */
#define RT_CONV_EXACT_FP32 1

/* 2-D convolution (cross-correlation), weights KCRS, bias K (may be NULL): TensorRT
 * addConvolution as called at sample_app/resnet18_2D_513x257_net.cpp:48-53 (no source in the
 * reference: TensorFlow conv2d semantics, scripts/tensorrt_model_builder.py:149-228).
 * x (N,Cin,Hin,Win) -> y (N,Cout,Hout,Wout), Hout = (Hin + 2*pad - KH)/stride + 1. */
int rt_conv2d_plan_create(rtConvPlan** plan, const rtConv2dDesc* desc, const void* weights_host,
                          const void* bias_host);
/* 2-D transposed convolution, weights (Cin,Cout,R,S), stride 2, 3x3: TensorRT addDeconvolution
 * (sample_app/resnet18_2D_513x257_net.cpp:722-727) = TF conv2d_transpose
 * (scripts/tensorrt_model_builder.py:230-288).  Hout = (Hin-1)*stride - 2*pad + KH. */
int rt_deconv2d_plan_create(rtConvPlan** plan, const rtConv2dDesc* desc, const void* weights_host,
                            const void* bias_host);

/* Fused residual block  y = act2(conv3x3(act1(conv3x3(x) + b1)) + b2 + x): the unit of the ResNet-18 feature towers
 * (reference resnet18_2D_513x257_net.cpp:66-575: resblockN_conv1, ELU plugin, resblockN_conv2, addElementWise(kSUM),
 * ELU plugin).  d1 / d2 describe the two addConvolution layers as rt_conv2d_plan_create would take them (d2->has_residual
 * = 1); RT_E_UNSUPPORTED unless both are 3x3, stride 1, pad 1, with <= 32 channels and equal input / output channel
 * counts.  Enqueue with residual = x (or NULL). */
int rt_resblock_plan_create(rtConvPlan** plan, const rtConv2dDesc* d1, const void* w1, const void* b1,
                            const rtConv2dDesc* d2, const void* w2, const void* b2);

/* Pre-split tensors between the blocks of a feature tower (not in the reference: TensorRT owns its internal formats): per sample
 * (C/8, H, pitch, [8 x fp16 hi | 8 x fp16 lo]) with x = hi + lo * 2^-11 -- the operands of the split-fp16 matrix instructions as stored
 * values, 4 bytes per element like the fp32 tensor it replaces (same pitch, same sample stride).  A block that READS one fills its LDS by
 * direct global -> LDS loads; a block that WRITES one splits its results in the epilogue.  Only the tower block takes them (32 -> 32 -> 32
 * channels, ELU after both convolutions of resblockN, reference resnet18_2D_513x257_net.cpp:66-575, on channel-interleaved fp32 tensors:
 * rt_conv_plan_set_layouts(plan, 1, 1, 1) first); rt_resblock_plan_supports_split says whether this plan does.  The skip connection of a
 * block with x_split is taken from the split tensor (22 bits). */
int rt_resblock_plan_supports_split(const rtConvPlan* plan);
int rt_resblock_plan_set_split(rtConvPlan* plan, int x_split, int y_split);

/* Row pitch (in elements, >= the row length; 0 = dense) of the input and of the output/residual planes of a 2-D
 * plan.  Not in the reference (TensorRT owns its internal layouts): lets the executor keep internal activations
 * 128-byte aligned per row.  Tensors are then (N, C, H, pitch) in memory with W valid columns. */
int rt_conv_plan_set_pitch(rtConvPlan* plan, int in_pitch, int out_pitch);
/* Per-sample strides in elements (0 = unchanged) of input / output / residual: a tensor may live inside a larger buffer,
 * e.g. as a channel range of the tensor TensorRT's addConcatenation would have copied it into
 * (reference resnet18_2D_513x257_net.cpp:612-615).  Call after rt_conv_plan_set_pitch. */
int rt_conv_plan_set_batch_strides(rtConvPlan* plan, int64_t x_bstride, int64_t y_bstride, int64_t r_bstride);

/* Storage type (RT_F32 / RT_F16) of the input and of the output + residual tensors of a 2-D plan: TensorRT's half2
 * mode (IBuilder::setHalf2Mode, sample_app/main.cpp:256-262) keeps activations in fp16 between layers.
 * fp16 -> fp16 (3x3 stride 1/2, transposed 3x3 stride 2): the plan's weights are re-packed as fp16 and the stored
 * values become the operands of the fp16 matrix instructions, accumulation stays fp32 (RT_NO_F16MMA=1 in the
 * environment keeps fp32 arithmetic).  fp32 -> fp16: the network's first layer (5x5 stride 2, <= 3 input channels)
 * rounds image and weights to fp16 and runs on the fp16 matrix instructions too, as TensorRT's half2 mode does; other
 * fp32 -> fp16 layers (direct-form kernels) and fp16 -> fp32 (last layer, small-output transposed kernel) compute in
 * fp32.  Other combinations return RT_E_UNSUPPORTED. */
int rt_conv_plan_set_io_types(rtConvPlan* plan, int x_dtype, int y_dtype);

/* Channel-interleaved tensors, (C/8, H, pitch, 8) per sample in fp16 and (C/4, H, pitch, 4) in fp32: one 16-byte slot
 * per pixel and channel group.
 * Not in the reference (TensorRT owns its internal layouts; its own fp16 formats are of this kind, PluginFormat
 * kNC2HW2 / kNHWC8 in NvInfer.h).  The 3x3 stride-1 kernels (fp32 Winograd, fp16 arithmetic) move such tensors in full
 * cache lines with a quarter of the memory instructions; the executor
 * uses the layout for tensors that only 3x3 stride-1 plans in fp16 arithmetic (and, as output, the first layer)
 * touch.  rt_conv_plan_supports_il8: which tensors of the plan may be interleaved (bit 0 input, bit 1 output, bit 2
 * residual, bit 3: an interleaved output only together with an interleaved input, bit 4: an interleaved input whose channel
 * count is padded up to a whole group -- the pad channels must hold finite values, bit 5: the input must stay planar fp32 (the
 * factored cost-volume fold of the first Conv3D); call it after
 * rt_conv_plan_set_io_types); rt_conv_plan_set_layouts: layout (0 planar, 1 interleaved) of
 * the input, the output and the residual tensor. */
int rt_conv_plan_supports_il8(const rtConvPlan* plan);
int rt_conv_plan_set_layouts(rtConvPlan* plan, int x_il8, int y_il8, int r_il8);

/* The soft-argmax that follows the last Conv3DTranspose of the 3-D models (disp_softargmax: reference lib/softargmax_plugin.cpp:167-205
 * over the volume lib/conv3d_transpose_plugin.cpp:137-166 wrote) inside that layer's launch: mode 1 = soft-argmax, 2 = soft-argmin over the
 * output depth, 0 = off.  rt_conv_enqueue then writes the (batch, 1, H, W) fp32 map to y (plain pitch W) and the (D, 1, H, W) volume is
 * never stored.  Only the depth-walking form of that layer has it -- one output channel, 32 input channels, fp16 channel-interleaved input,
 * fp32 output, no residual; any other plan returns RT_E_UNSUPPORTED and stays as it is (the caller then runs rt_softargmax on the volume).
 * Call it last: rt_conv_plan_set_io_types / rt_conv_plan_set_layouts switch it off. */
int rt_conv_plan_set_softarg(rtConvPlan* plan, int mode);

typedef struct rtConv3dDesc {
    int C, K;               /* conv: input channels C, output channels K.  Transposed op: K = INPUT   */
                            /* channels (tensor KDHW), C = OUTPUT channels (tensor DCHW)             */
    int D, H, W;            /* conv: input dims (D,C,H,W); transposed: OUTPUT dims (D,C,H,W)         */
    int kernel[3];          /* (V,R,S): filter is (K,V,C,R,S); R = S in {1,3}                        */
    int stride[3];          /* (d,h,w), h == w                                                      */
    int pad_start[3];       /* (d,h,w) -- what the reference hands to cuDNN                         */
    int pad_end[3];         /* validated like lib/conv3d_plugin.cpp:43-49, otherwise unused          */
    int act;                /* RT_ACT_* (0 at the plugin boundary; used by the fusing executor)     */
    int out_dchw;           /* conv: write (Do,K,Ho,Wo) instead of (K,Do,Ho,Wo); transposed: write (C,D,H,W)  */
                            /* instead of (D,C,H,W) -- the Transform plugin that follows, in the same pass  */
    int has_residual;       /* residual tensor: shaped like the output; for the transposed op always (D,C,H,W) */
    int dtype;
    int out_depth;          /* transposed only: keep output depth slices [0, out_depth) (0 = all) -- the      */
                            /* Slice plugin that follows an even-depth conv3d_transpose, in the same pass      */
    int in_pad_end;         /* conv only: the last in_pad_end of the D input slices are zeros that do not exist  */
                            /* in memory (x is (D - in_pad_end, C, H, W)) -- the Pad plugin emitted before every  */
                            /* stride-2 Conv3D (scripts/tensorrt_model_builder.py:331-345), in the same pass     */
    int cv_fold;            /* conv only, executor: F > 0 = the input is the DEFAULT COST VOLUME of two (F,H,W) feature  */
                            /* maps (C == 2F; CostVolumePlugin kDefault, lib/kernels.cu:50-97) that is never built:     */
                            /* x points to the (2F, H, W) tensor [left | right] and slice d of the volume is gathered   */
                            /* as cv[d, 0:F] = L, cv[d, F:2F, y, x] = R[:, y, x - d] (0 for x < d)                       */
    int flags;              /* RT_CONV_* option bits (see rtConv2dDesc), 0 = defaults                               */
} rtConv3dDesc;

/* TensorFlow-compatible 3-D convolution.  x (N, D,C,H,W) , w (K,V,C,R,S) 3x3x3 -> y (N, K,Do,Ho,Wo).
 * Replaces Conv3DPlugin::enqueue -> cudnnConvolutionForward on the (D*C)-merged descriptor +
 * cudnnAddTensor bias (lib/conv3d_plugin.cpp:187-216, lib/conv_utils.cpp:27-32,58-72). */
int rt_conv3d_plan_create(rtConvPlan** plan, const rtConv3dDesc* desc, const void* weights_host,
                          const void* bias_host);
/* TensorFlow-compatible 3-D transposed convolution.  y (N, K,Dy,Hy,Wy), w (K,V,C,R,S) -> x (N, D,C,H,W),
 * bias per C.  Replaces Conv3DTransposePlugin::enqueue -> cudnnConvolutionBackwardData +
 * addDBiasTo3DConvKernel (lib/conv3d_transpose_plugin.cpp:205-243, lib/kernels.cu:292-335).
 * in_dims = (Dy,Hy,Wy) of the input. */
int rt_conv3d_transpose_plan_create(rtConvPlan** plan, const rtConv3dDesc* desc, const int in_dims[3],
                                    const void* weights_host, const void* bias_host);

/* 1 when the library was built with -DRT_EXPERIMENTAL: the measured-and-rejected kernel families (persistent split kernel, per-tile fused
 * residual block, 8-row / 8-wave tiles, Winograd on interleaved tensors) are then compiled in and selectable through development knobs.
 * The product build returns 0; the CPU test tier's emulator build returns 1. */
int rt_has_experimental(void);

/* The domain of a plan's arithmetic.  The default fp32 path multiplies 22-bit fp16 splits on the fp16 matrix pipe: an input value with
 * |x| >= 65504 (or a non-finite one) becomes inf / NaN in the result -- loud, but far from its cause.  rt_conv_plan_input_limit gives the
 * bound a plan needs (65504 for split / fp16-operand plans, +inf for RT_CONV_EXACT_FP32 and the small direct kernels);
 * rt_check_range scans a device tensor of `rows` rows with `valid` leading elements out of `pitch` each (dense: rows = 1, valid = pitch = n):
 * max |x| and the number of elements with |x| >= limit or non-finite.  Blocking.  IExecutionContext::setDebugSync(true) /
 * rt_net_set_debug make the executor run it on the input of every such launch and fail the execute() with the layer's name. */
int rt_conv_plan_input_limit(const rtConvPlan* plan, float* limit);
int rt_check_range(const void* x, int64_t rows, int64_t valid, int64_t pitch, int dtype, float limit, float* max_abs, int64_t* violations,
                   rtStream stream);

/* Order-independent 64-bit checksum of `bytes` (a multiple of 4) of device memory, written to the device word `out_dev` on `stream`
 * (asynchronous).  Two buffers with the same bits give the same value; the executor's launch trace (rt_net_set_launch_trace) hashes every
 * launch's output with it so that two passes over the same input can be compared launch by launch without copying tensors. */
int rt_hash_buffer(const void* x, size_t bytes, unsigned long long* out_dev, rtStream stream);

/* Output dims of a plan: 2-D -> (Cout,Hout,Wout,1); 3-D -> 4 dims in the order they are written. */
int rt_conv_plan_out_dims(const rtConvPlan* plan, int dims[4]);
/* Run: x, y (and residual, shaped like y, or NULL) are device pointers for `batch` samples. */
int rt_conv_enqueue(const rtConvPlan* plan, const void* x, void* y, const void* residual, int batch,
                    rtStream stream);
/* The same with launch hints (0 = rt_conv_enqueue).  RT_HINT_THROUGHPUT: the caller keeps several launches in flight on the device
 * (execution contexts with one stream each, TensorRT's `trtexec --streams` set-up; IExecutionContext::setExecutionStreams(1)): kernels
 * may then trade the duration of one launch for device time per result -- the streaming residual block walks 64-row instead of 32-row
 * segments (fewer pipeline fill / drain steps per row, half the workgroups per launch); without the hint, launches that would leave a
 * SIMD a single wave split their contraction over wave groups (split-K: another fp32 summation order).  Results are deterministic for
 * a given (hints, device CU count) and agree across hints to fp32 rounding (<= 1e-5 on the networks' outputs), not bit for bit. */
#define RT_HINT_THROUGHPUT 1
int rt_conv_enqueue_hint(const rtConvPlan* plan, const void* x, void* y, const void* residual, int batch,
                         rtStream stream, int hints);
/* The first layer of both feature towers in one launch: samples 0 .. batch - 1 from x (left images), batch .. 2 batch - 1 from x2 (right
 * images -- the reference's two input bindings, sample_app/main.cpp:290-300), y = 2 * batch samples.  The towers share their weights, so
 * this is the [left | right] launch the executor makes of every tower layer; only first-layer plans (5x5 stride 2, <= 3 input channels,
 * rt_conv_plan_supports_twin_input) have it. */
int rt_conv_plan_supports_twin_input(const rtConvPlan* plan);
int rt_conv_enqueue_twin_input(const rtConvPlan* plan, const void* x, const void* x2, void* y, int batch, rtStream stream, int hints);

/* Scratch a plan's launches need for `batch` samples, in bytes (0 for most plans; the first Conv3D over a folded cost volume in its
 * factored form keeps four small maps per sample).  The caller owns it -- an execution context passes its workspace, as TensorRT hands a
 * plugin's getWorkspaceSize() bytes to enqueue (reference lib/conv3d_plugin.cpp:179-185, 187-190) -- so that contexts sharing a plan do
 * not share scratch: 16-byte aligned device memory of at least that size, private to the stream until the launches have run.
 * rt_conv_enqueue / _hint on such a plan use blocks owned by the plan instead, one per stream they are called with (safe across streams;
 * a block grows after its stream has drained, which a stream capture cannot record: capturing callers pass a workspace). */
size_t rt_conv_plan_workspace_bytes(const rtConvPlan* plan, int batch);
int rt_conv_enqueue_ws(const rtConvPlan* plan, const void* x, void* y, const void* residual, int batch, void* workspace,
                       size_t workspace_bytes, rtStream stream, int hints);
int rt_conv_plan_destroy(rtConvPlan* plan);

/* ---- multi-GPU: RCCL communicator and byte broadcast ---------------------------------------------------------
 * Stereo pairs are independent (the reference is single-GPU, batch 1: sample_app/main.cpp:260, 303-305), so ranks share
 * nothing but the weight-file image: rank `root` reads trt_weights.bin, every other rank receives it over RCCL / xGMI
 * (ncclBroadcast) at start-up, and no collective touches the data path.  librccl is loaded on first use (dlopen), so
 * single-GPU users never pay for it.  One communicator per (process or thread, device): call rt_set_device first.
 *   rank 0:  rt_comm_unique_id(id)  -> ship the 128 bytes to the other ranks by any means (file, socket, MPI, torchrun's store)
 *   all:     rt_comm_init_rank(&comm, world, rank, id)          (ncclCommInitRank)
 *   or:      rt_comm_adopt(&comm, existing ncclComm_t)           (a communicator the host application already has; not destroyed)
 *   or:      rt_comm_init_all(comms, ndev, devices)              (one process driving several devices: ncclCommInitAll)
 *   all:     rt_comm_broadcast(comm, host_buffer, bytes, root, stream)   blocking; bytes must agree on every rank
 * Calls of one process that must progress together (several comms driven from one thread) go between
 * rt_comm_group_start / rt_comm_group_end. */
typedef struct rtComm rtComm;
#define RT_COMM_ID_BYTES 128
int rt_comm_unique_id(void* id_bytes);
int rt_comm_init_rank(rtComm** comm, int world, int rank, const void* id_bytes);
int rt_comm_init_all(rtComm** comms, int ndev, const int* devices);
int rt_comm_adopt(rtComm** comm, void* nccl_comm);
int rt_comm_info(const rtComm* comm, int* world, int* rank);
int rt_comm_broadcast(rtComm* comm, void* host_buf, size_t bytes, int root, rtStream stream);
int rt_comm_group_start(void);
int rt_comm_group_end(void);
int rt_comm_destroy(rtComm* comm);

#ifdef __cplusplus
}
#endif
#endif /* RT_STEREO_H */
