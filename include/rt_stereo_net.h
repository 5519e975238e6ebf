/*
 * rt_stereo_net.h -- whole-network C ABI of the Stereo DNN inference path on MI355X.
 *
 * What sample_app/main.cpp:136-340 and ros/packages/stereo_dnn_ros/src/stereo_dnn_ros_node.cpp:224-377 of
 * the reference do with TensorRT objects (read trt_weights.bin, build the network through the
 * IPluginContainer API, build an engine, create a context, execute on device buffers) behind five
 * plain-C calls, so that non-C++ hosts (ctypes in bench.py / tests, cgo, JNI ...) can drive the same
 * code path.  Implemented by redtail_amd/csrc/host/net_capi.cpp on top of the NvInfer.h shim.
 */
#ifndef RT_STEREO_NET_H
#define RT_STEREO_NET_H

#include <stddef.h>
#include <stdint.h>

#include "rt_stereo.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtStereoNet rtStereoNet;

/* model_type strings of sample_app/main.cpp:155-161 */
enum { RT_MODEL_RESNET18_2D = 0, RT_MODEL_NVSMALL = 1, RT_MODEL_NVTINY = 2, RT_MODEL_RESNET18 = 3 };

/* Build an engine for `width` x `height` images (any size = 1 mod 8 for ResNet-18 2D).
 * weights_dtype: RT_F32 / RT_F16 = element type of the weight blob (trt_weights.bin / trt_weights_fp16.bin,
 * layout of scripts/tensorrt_model_builder.py:52-60).  Activations are fp32.  max_disp <= 0 selects the
 * model's default half-resolution disparity range (48 / 48 / 24 / 68). */
int rt_net_create(rtStereoNet** net, int model, int width, int height, int max_batch, int weights_dtype,
                  int max_disp, const char* weights_path);
/* Same, from an in-memory image of the weight file (what rank 0 broadcasts over RCCL). */
int rt_net_create_from_memory(rtStereoNet** net, int model, int width, int height, int max_batch, int weights_dtype,
                              int max_disp, const void* blob, size_t bytes);

/* Multi-GPU start-up without Python: every rank of `comm` (rt_stereo.h: rt_comm_init_rank / rt_comm_adopt / rt_comm_init_all)
 * calls this on its own device; rank `root` passes the weight-file image, the others pass NULL / 0 and receive it over RCCL
 * (ncclBroadcast: first its size, then its bytes), then every rank builds the same engine.  What redtail_amd/parallel.py does
 * through torch.distributed, for hosts that have no torch (apps/stereo_throughput.cpp).  comm == NULL: world of one rank. */
int rt_net_create_broadcast(rtStereoNet** net, int model, int width, int height, int max_batch, int weights_dtype,
                            int max_disp, const void* blob, size_t bytes, rtComm* comm, int root);
/* crc32 (zlib polynomial) of the weight-file image the engine was built from: every rank prints it, they must agree */
int rt_net_weights_crc32(const rtStereoNet* net, uint32_t* crc);
/* The image itself (owned by the engine, valid until rt_net_destroy): a rank that received it by broadcast builds its further
 * execution contexts from it (rt_net_create_from_memory). */
int rt_net_weights_image(const rtStereoNet* net, const void** data, size_t* bytes);

/* Everything above in one call, options as a struct (zero-initialise, then set what is needed): weights from `weights_path` or from the
 * image `blob` / `bytes` (the root rank's when `comm` is set, see rt_net_create_broadcast); flags: RT_CONV_EXACT_FP32 keeps every 2-D
 * convolution on the fp32 fmaf-chain kernels (IBuilder::setExactFp32Mode). */
typedef struct rtNetOptions {
    int model, width, height, max_batch;
    int weights_dtype;         /* RT_F32 / RT_F16 */
    int max_disp;              /* <= 0: the model's default */
    const char* weights_path;  /* or NULL */
    const void* blob;          /* or NULL */
    size_t bytes;
    unsigned flags;            /* RT_CONV_EXACT_FP32 */
    rtComm* comm;              /* or NULL: no broadcast */
    int root;
} rtNetOptions;
int rt_net_create_opt(rtStereoNet** net, const rtNetOptions* options);

/* left/right: device (N,3,H,W) fp32 in [0,1]; disp: device (N,1,H,W) fp32 (ResNet-18 2D: disparity / width;
 * 3-D models: pixels).  stream == NULL: synchronous (IExecutionContext::execute); otherwise asynchronous on
 * that HIP stream (IExecutionContext::enqueue). */
int rt_net_execute(rtStereoNet* net, const void* left, const void* right, void* disp, int batch, rtStream stream);

/* What rt_net_execute_frames writes into `disp`:
 *   RT_DISP_NET         fp32, what rt_net_execute writes (ResNet-18 2D: disparity / width; 3-D models: pixels)
 *   RT_DISP_PIXELS_F32  fp32 disparity in pixels: the ROS node's 32FC1 output (stereo_dnn_ros_node.cpp:81, 89); the sample app's
 *                       scale per model (sample_app/main.cpp:325-327): x width for ResNet-18 2D, x 1 for NVSmall / NVTiny / ResNet-18 3D
 *   RT_DISP_KITTI_U16   uint16, the sample app's 16-bit PNG values (main.cpp:321-330): rt_disparity_to_u16(disp, 256 x that scale) */
/* (the enum itself is in rt_stereo.h, beside rt_lr_consistency, which writes the same three forms) */
/* The ROS node's per-frame path (stereo_dnn_ros_node.cpp:60-103) in one call: left_u8 / right_u8 are device batches of camera frames
 * (rt_stereo.h: rt_preprocess_frames_u8 -- src_h x src_w pixels, rows src_step bytes apart, RT_ENC_* encoding), pre-processed to the
 * network's size into fp32 buffers the net owns, run as rt_net_execute does into a disparity the net owns, then written to `disp` as
 * `disp_kind` says.  The engine's three bindings never change, so graph mode (rt_net_set_graph) replays one graph whatever frame and
 * output pointers the caller rotates through.  stream == NULL: synchronous (pre-processing on the NULL stream, IExecutionContext::execute,
 * the output step, then a synchronisation); otherwise everything is asynchronous on that stream.  As with rt_net_execute, calls on one
 * net are ordered by the caller.  Errors (batch > max_batch, unknown kind or encoding, unsupported scale factors) write nothing. */
int rt_net_execute_frames(rtStereoNet* net, const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step,
                          int encoding, void* disp, int disp_kind, int batch, rtStream stream);
/* rt_net_execute_frames plus a left-right consistency check (rt_stereo.h: rt_preprocess_frames_u8_lr, rt_lr_consistency, where the check
 * is defined): the frames are pre-processed once into the net-owned inputs together with their mirrored, swapped twins, the engine runs
 * ONE pass at batch 2 * batch (so 2 * batch <= max_batch is required), and rt_lr_consistency writes the caller's buffers:
 *   disp        (batch,1,H,W) in disp_kind, inconsistent pixels = 0 (RT_DISP_KITTI_U16: a consistent 0 is raised to 1, the KITTI rule)
 *   mask_u8     (batch,1,H,W) uint8, 255 = consistent; or NULL        disp_right  the right view's disparity in disp_kind; or NULL
 *   valid_count `batch` uint64 on the device, consistent pixels per image; or NULL
 * max_diff_px >= 0 is the largest |dL - dR| in pixels that counts as consistent (OpenCV's disp12MaxDiff).  The cost is the engine pass
 * at twice the batch.  The bindings are those of rt_net_execute_frames: in graph mode a net may alternate between the two calls, each
 * engine batch keeps its own graph.  Streams, synchronisation and errors (which write nothing) as rt_net_execute_frames. */
int rt_net_execute_frames_lr(rtStereoNet* net, const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step,
                             int encoding, void* disp, int disp_kind, void* mask_u8, void* disp_right, void* valid_count,
                             float max_diff_px, int batch, rtStream stream);
/* The DNN node's and the viz node's messages from one call: rt_net_execute_frames(..., RT_DISP_PIXELS_F32) -- or, when max_diff_px >= 0,
 * rt_net_execute_frames_lr(..., RT_DISP_PIXELS_F32, mask_u8, NULL, valid_count, max_diff_px) -- followed by rt_viz_mosaic_u8
 * (rt_stereo.h) of the same frames and of the disparity just written, on the same stream: one more launch, no new buffers.
 *   disp_px   (batch,1,H,W) fp32 disparity in pixels (the DNN node's 32FC1 message)
 *   viz_rgb8  per image a (2H) x (2W) rgb8 panel, rows viz_step >= 6W bytes apart (the viz node's rgb8 message); max_disp: its colour
 *             range (the node uses 96).  A checked disparity is 0 at inconsistent pixels, which is black in both disparity panels.
 * max_diff_px < 0: no check, mask_u8 and valid_count must be NULL; a NaN is an error.  The panel is launched outside the engine's graph,
 * like the pre-processing and the output step, so in graph mode frame, disparity and panel pointers may rotate.  Streams and
 * synchronisation as the two calls; every error (theirs, a short viz_step, a max_disp that is not a finite number > 0) writes nothing. */
int rt_net_execute_frames_viz(rtStereoNet* net, const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step,
                              int encoding, void* disp_px, void* viz_rgb8, int64_t viz_step, float max_disp, float max_diff_px,
                              void* mask_u8, void* valid_count, int batch, rtStream stream);

/* Frames of any size in, disparity at the frame's size out, from one call; options travel in a struct that can grow.
 * Launches: the front end (rt_preprocess_frames_u8 / _lr, or rt_preprocess_frames_u8_cv), the engine (one pass, batch or 2 * batch with
 * a check), then
 *   RT_GEOM_NET    as rt_net_execute_frames (copy / scale / 16-bit) or, with a check, rt_lr_consistency into the caller's buffers;
 *   RT_GEOM_FRAME  the network's pixels (rt_disparity_scale by the model's scale, skipped where that is 1; with a check
 *                  rt_lr_consistency in network geometry, in pixels, with its mask) into buffers the net owns, then
 *                  rt_disparity_to_frame into the caller's (batch,1,src_h,src_w) buffers, which carries the mask over.
 * The result is bit-identical to these op-level calls made by hand around rt_net_execute; with RT_RESIZE_AREA_DOWN and RT_GEOM_NET it
 * is rt_net_execute_frames / rt_net_execute_frames_lr on the same arguments, refusals included.  The network-geometry disparity and mask
 * are made on first use for max_batch, like the inputs.  Front and back end run outside the engine's graph, so frame and output
 * pointers may rotate in graph mode.  stream == NULL: synchronous.  RT_GEOM_FRAME with RT_DISP_NET: RT_E_UNSUPPORTED.  A wrong
 * struct_bytes, an unknown enum value, a NaN max_diff_px, mask_u8 / valid_count without a check, batch (2 * batch with a check) beyond
 * max_batch, and whatever the op-level calls refuse: error before anything is written. */
enum { RT_RESIZE_AREA_DOWN = 0 /* as rt_net_execute_frames: refuses up-scaling */, RT_RESIZE_CV_AREA = 1 /* rt_preprocess_frames_u8_cv */ };
enum { RT_GEOM_NET = 0, RT_GEOM_FRAME = 1 };
typedef struct rtFrameCall {
    size_t struct_bytes;       /* sizeof(rtFrameCall): lets the struct grow */
    const void* left_u8;       /* device frames as rt_net_execute_frames takes them */
    const void* right_u8;
    int src_h, src_w;
    int64_t src_step;
    int encoding;              /* RT_ENC_* */
    int resize;                /* RT_RESIZE_* */
    void* disp;
    int disp_kind;             /* RT_DISP_* */
    int geometry;              /* RT_GEOM_NET: (batch,1,net_h,net_w).  RT_GEOM_FRAME: (batch,1,src_h,src_w), the frame's pixels */
    float max_diff_px;         /* < 0: no left-right check; >= 0: as rt_net_execute_frames_lr, 2 * batch <= max_batch */
    void* mask_u8;             /* optional, only with a check; in the geometry of `disp` */
    void* valid_count;
    int batch;
} rtFrameCall;
int rt_net_execute_frames_ex(rtStereoNet* net, const rtFrameCall* call, rtStream stream);

/* rt_net_execute_frames_ex in frame geometry with a depth image and / or a point cloud beside (or instead of) the disparity: the same
 * sequence -- front end, one engine pass (2 * batch with a check), rt_disparity_scale or rt_lr_consistency into the net-owned
 * network-geometry buffers -- with rt_disparity_to_points (rt_stereo.h, where depth, cloud and their validity are defined) in the place of
 * rt_disparity_to_frame.  The result is bit-identical to those op-level calls made by hand around rt_net_execute.
 *   call   as rt_net_execute_frames_ex takes it.  call->geometry must be RT_GEOM_FRAME: depth and cloud exist in the camera's own geometry
 *          only, so the caller never rescales intrinsics; RT_GEOM_NET: RT_E_UNSUPPORTED.  call->disp may be NULL if `out` requests
 *          something; otherwise disp_kind, mask_u8 and valid_count (the check's validity, carried over) are RT_GEOM_FRAME's.
 *   out    camera: the CAMERA's calibration in the frame's geometry (src_h x src_w), used as it is; depth (batch,1,src_h,src_w) in
 *          depth_kind, points (organised cloud), points_compact + count (valid points only; count = points that pass the check AND
 *          the depth range), each or NULL.  The colour of a cloud is call->left_u8 itself.  out == NULL: rt_net_execute_frames_ex.
 * The workspace of a compact cloud is a buffer the net owns, made on first use for max_batch.  The op runs outside the engine's graph, so
 * every pointer may rotate in graph mode; stream == NULL: synchronous.  Whatever rt_net_execute_frames_ex or rt_disparity_to_points
 * refuse, and a wrong struct_bytes of either struct: error before anything is written. */
typedef struct rtDepthCall {
    size_t struct_bytes;       /* sizeof(rtDepthCall) */
    rtStereoCamera camera;
    float min_depth, max_depth;
    void* depth;
    int depth_kind;            /* RT_DEPTH_* */
    void* points;
    void* points_compact;
    void* count;
} rtDepthCall;
int rt_net_execute_frames_3d(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out, rtStream stream);

/* RAW camera frames in: rectification in front of rt_net_execute_frames_3d (rt_net_execute_frames_ex with out == NULL).
 * call->left_u8 / right_u8 are raw frames (image_raw).  One rt_rectify_frames_u8 launch (rt_stereo.h, where map and sampler are defined)
 * makes rectified frames of the same size and encoding -- dense buffers the net owns, made on first use for max_batch and regrown when a
 * larger frame arrives, or the caller's left_rect_u8 / right_rect_u8 (image_rect_color), rows rect_step bytes apart -- and the call then
 * is rt_net_execute_frames_3d(net, &call2, out, stream) with call2 = *call, its frame pointers and step replaced by the rectified ones.
 * Composition is the definition: every output is bit-identical to those two calls made by hand, the cloud's colour is the rectified
 * left pixel, out->camera is the calibration P describes, and whatever the wrapped call refuses is refused here.  All checks of all three
 * structs are made before the first launch, so an error writes nothing.  Also refused: a wrong struct_bytes, one of left_rect_u8 /
 * right_rect_u8 without the other, a rect_step shorter than a row (or not 0 with NULL), a non-finite camera field, a rectified buffer
 * that is the raw one.  The rectify launch runs outside the engine's graph, so every pointer may rotate in graph mode; stream == NULL:
 * synchronous. */
typedef struct rtRectifyCall {
    size_t struct_bytes;                 /* sizeof(rtRectifyCall) */
    rtRectifyCamera left, right;
    void* left_rect_u8;                  /* optional: receive the rectified frames (image_rect_color), src_h x src_w, call->encoding ... */
    void* right_rect_u8;                 /* ... both or neither; NULL: buffers the net owns */
    int64_t rect_step;                   /* row step of those two; 0 with NULL */
} rtRectifyCall;
int rt_net_execute_frames_raw(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out /* or NULL */, const rtRectifyCall* rect,
                              rtStream stream);

/* The calls above with a speckle filter (rt_stereo.h: rt_disparity_speckle, where live pixels, adjacency, components and what is written
 * are defined; stereo_image_proc's speckle_size / speckle_range) where it belongs: in network geometry, in front of the resampling.
 *   speckle == NULL: rt_net_execute_frames_raw on the same arguments; with rect == NULL rt_net_execute_frames_3d, with out == NULL as well
 *                    rt_net_execute_frames_ex; refusals included.
 *   speckle != NULL: call->geometry must be RT_GEOM_FRAME (RT_GEOM_NET: RT_E_UNSUPPORTED, as for depth).  The sequence is the existing one
 *                    with ONE rt_disparity_speckle(max_size, max_diff_px) between the step that makes network-geometry pixels and
 *                    rt_disparity_to_frame / rt_disparity_to_points: behind rt_lr_consistency in place on the net-owned disparity and mask;
 *                    without a check with a NULL input mask into those two buffers -- behind rt_disparity_scale in place, for the 3-D
 *                    models (whose output is pixels already) out of place from the engine's output.  The back end therefore always gets
 *                    a mask, and call->mask_u8 / call->valid_count are legal without a check: they then say which pixels the filter kept.
 * Composition is the definition: every output is bit-identical to those op-level calls made by hand around rt_net_execute.  The filter
 * costs launches and no engine work.  Its workspace is a buffer the net owns, made on first use for max_batch.  It runs outside the
 * engine's graph, so every pointer may rotate in graph mode; stream == NULL: synchronous.  All checks of all four structs are made before
 * the first launch, so an error writes nothing: whatever the wrapped calls refuse (mask_u8 / valid_count with neither a check nor a filter
 * included), a wrong struct_bytes, max_size < 0, a max_diff_px that is negative, NaN or infinite. */
typedef struct rtSpeckleCall {
    size_t struct_bytes;       /* sizeof(rtSpeckleCall) */
    int max_size;              /* components of at most this many network-geometry pixels are removed (speckle_size); 0 removes nothing */
    float max_diff_px;         /* largest step between neighbours of one component, network-geometry pixels (speckle_range) */
} rtSpeckleCall;
int rt_net_execute_frames_filtered(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out /* or NULL */,
                                   const rtRectifyCall* rect /* or NULL */, const rtSpeckleCall* speckle /* or NULL */, rtStream stream);

/* What the camera really sends in: mono, Bayer or YUV 4:2:2 frames (rt_stereo.h: RT_WIRE_*, rt_decode_frames_u8, where every conversion is
 * defined) in front of rt_net_execute_frames_filtered.
 *   decode == NULL: rt_net_execute_frames_filtered on the same arguments, refusals and error texts included.
 *   decode != NULL: call->left_u8 / right_u8 are WIRE frames of decode->wire_encoding, rows call->src_step bytes apart, and call->encoding is
 *                   the RT_ENC_* encoding to decode into.  One rt_decode_frames_u8 launch makes colour frames of the same size -- dense
 *                   buffers the net owns, made on first use for max_batch and regrown when a larger frame arrives, or the caller's
 *                   left_color_u8 / right_color_u8 (image_color), rows color_step bytes apart -- and the call then is
 *                   rt_net_execute_frames_filtered(net, &call2, out, rect, speckle, stream) with call2 = *call, its frame pointers and step
 *                   replaced by the decoded ones.  Debayering comes before rectification, as in image_proc; rectified frames, the cloud's
 *                   colour and everything else downstream see call->encoding.
 * Composition is the definition: every output is bit-identical to those two calls made by hand.  All checks of all five structs are made
 * before the first launch -- the decode launch -- so an error writes nothing: whatever the wrapped call and its front end refuse (with
 * call->src_step held against the WIRE pixel size: bad dimensions, a short step, up-scaling under RT_RESIZE_AREA_DOWN, factors outside
 * [1/6, 6]), whatever rt_decode_frames_u8 refuses, a wrong struct_bytes, one of left_color_u8 / right_color_u8 without the other, a
 * color_step shorter than a row (or not 0 with NULL), a colour buffer that is a wire buffer or a rectified buffer.  The decode launch runs
 * outside the engine's graph, so every pointer may rotate in graph mode; stream == NULL: synchronous.  The other rt_net_execute_frames*
 * entries go on refusing wire encodings: for the viz panel of a Bayer camera, decode with rt_decode_frames_u8 and pass the result on. */
typedef struct rtDecodeCall {
    size_t struct_bytes;        /* sizeof(rtDecodeCall) */
    int wire_encoding;          /* RT_WIRE_*: what call->left_u8 / right_u8 hold, rows call->src_step bytes apart */
    void* left_color_u8;        /* optional: receive the decoded frames (image_color), src_h x src_w in call->encoding ... */
    void* right_color_u8;       /* ... both or neither; NULL: dense buffers the net owns */
    int64_t color_step;         /* row step of those two; 0 with NULL */
} rtDecodeCall;
int rt_net_execute_frames_camera(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out /* or NULL */,
                                 const rtRectifyCall* rect /* or NULL */, const rtSpeckleCall* speckle /* or NULL */,
                                 const rtDecodeCall* decode /* or NULL */, rtStream stream);

/* What a planner can take: rt_net_execute_frames_camera with the cloud put on a voxel grid (rt_stereo.h: rt_points_voxel_grid, where cells,
 * sums, the emitted record and its order are defined; pcl::VoxelGrid, the node behind stereo_image_proc/point_cloud2).
 *   voxel == NULL: rt_net_execute_frames_camera on the same arguments, refusals and error texts included.
 *   voxel != NULL: `out` is required -- it carries the camera and the depth range -- and may have every output pointer NULL: "no output
 *                  requested" is satisfied by the voxels.  The sequence is the existing one with ONE
 *                  rt_points_voxel_grid(grid, min_points) behind rt_disparity_to_points.  Its input cloud is the caller's out->points
 *                  (read with count == NULL) or, failing that, out->points_compact with out->count, where one was asked for; otherwise an
 *                  organised cloud in a buffer the net owns, made on first use and regrown when a larger frame arrives.  The choice cannot
 *                  be observed: the op's result is a function of the set of valid points, which is the same in all three.
 *                  voxels / capacity / count / cell_u32 / n_u32 are the op's voxels / out_capacity / out_count / out_cell_u32 /
 *                  out_n_u32, capacity per image.
 * Composition is the definition: every output is bit-identical to rt_net_execute_frames_camera followed by rt_points_voxel_grid by hand.
 * The voxel workspace is a buffer the net owns, grown on demand.  The op runs outside the engine's graph, so every pointer may rotate in
 * graph mode; stream == NULL: synchronous.  All checks of all six structs are made before the first launch, so an error writes nothing:
 * whatever the wrapped call refuses, whatever rt_points_voxel_grid refuses (a frame of more than 2^23 pixels included), a wrong
 * struct_bytes, a NULL `out`, voxel buffers that overlap the cloud they are made from. */
typedef struct rtVoxelCall {
    size_t struct_bytes;       /* sizeof(rtVoxelCall) */
    rtVoxelGrid grid;
    int min_points;
    void* voxels;              /* rt_points_voxel_grid's outputs; capacity per image */
    int capacity;
    void* count;
    void* cell_u32;            /* optional */
    void* n_u32;               /* optional */
} rtVoxelCall;
int rt_net_execute_frames_voxels(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out, const rtRectifyCall* rect /* or NULL */,
                                 const rtSpeckleCall* speckle /* or NULL */, const rtDecodeCall* decode /* or NULL */,
                                 const rtVoxelCall* voxel /* or NULL */, rtStream stream);

/* Per-launch timing through nvinfer1::IProfiler (single stream, one event pair per launch):
 * writes "name<TAB>milliseconds\n" lines into buf.  Returns 0 or an error. */
int rt_net_profile(rtStereoNet* net, const void* left, const void* right, void* disp, int batch, char* buf,
                   size_t buf_bytes);

/* Engine plan: ICudaEngine::serialize() (sample_app/main.cpp:269-275).  buf == NULL queries the size.  Fails for
 * networks with non-serialisable plugins (the 3-D models), as the reference does. */
int rt_net_serialize(rtStereoNet* net, void* buf, size_t buf_bytes, size_t* plan_bytes);
/* IRuntime::deserializeCudaEngine(plan, size, &StereoDnnPluginFactory) + createExecutionContext
 * (sample_app/main.cpp:198-220; lib/internal_utils.cpp:289-313). */
int rt_net_create_from_plan(rtStereoNet** net, const void* plan, size_t plan_bytes);
int rt_net_num_layers(const rtStereoNet* net);     /* layers of the network definition  */
/* HIP streams the context issues its launches on: 2 (default) = the right-image encoder on a second stream, best for one
 * context (latency); 1 = everything on the caller's stream, best when several handles are kept busy side by side
 * (IExecutionContext::setExecutionStreams, an extension of the NvInfer.h subset; bench.py uses 1 with its six contexts). */
int rt_net_set_streams(rtStereoNet* net, int streams);
/* Graph mode (IExecutionContext::setGraphMode, an extension): the second rt_net_execute with the same device pointers, batch and stream
 * is captured as a hipGraph (rt_stereo.h: rt_graph_*), every further one is a single graph launch; other pointers capture another graph.
 * Off by default (the host is not the bottleneck of this path). */
int rt_net_set_graph(rtStereoNet* net, int on);
/* Debug mode (IExecutionContext::setDebugSync): every launch is synchronised and the input of every fp16-pipe convolution is range-checked
 * first (rt_check_range): an execute() whose activations leave the fp16-split domain fails with the layer's name in rt_net_last_error(). */
int rt_net_set_debug(rtStereoNet* net, int on);
/* Launch trace (IExecutionContext::setLaunchTrace, a debugging aid): while on, the output of every launch is hashed on the launch's own
 * stream (rt_stereo.h: rt_hash_buffer).  rt_net_read_launch_trace waits for the last pass and returns one value per launch (count, or -1);
 * two passes over the same input must agree launch by launch -- the first index that differs names the kernel that deviated.
 * rt_net_launch_name: the launch's layer name; rt_net_read_launch_output: its output tensor as stored (host == NULL: size in bytes). */
int rt_net_set_launch_trace(rtStereoNet* net, int on);
int rt_net_read_launch_trace(rtStereoNet* net, unsigned long long* hashes, int max);
const char* rt_net_launch_name(const rtStereoNet* net, int launch);
long long rt_net_read_launch_output(rtStereoNet* net, int launch, void* host, long long bytes);
int rt_net_num_launches(const rtStereoNet* net);   /* kernel launches after fusion       */
int rt_net_destroy(rtStereoNet* net);
const char* rt_net_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
