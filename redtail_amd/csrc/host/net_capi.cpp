// Whole-network C ABI (include/rt_stereo_net.h): weight-file parsing, network/engine/context life cycle.
#include "rt_stereo_net.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "networks.h"
#include "redtail_tensorrt_plugins.h"

using namespace nvinfer1;
using namespace redtail::tensorrt;

namespace {

thread_local std::string g_net_err;

class NetLogger : public ILogger {
public:
    NetLogger() {
        const char* e = getenv("RT_LOG_LEVEL");
        level_ = e ? atoi(e) : 1;
    }
    void log(Severity severity, const char* msg) override {
        if ((int)severity <= (int)Severity::kERROR) last_error = msg;
        if ((int)severity > level_) return;
        static const char* tag[] = {"INTERNAL_ERROR", "ERROR", "WARNING", "INFO"};
        fprintf(stderr, "[redtail_amd %s] %s\n", tag[(int)severity & 3], msg);
    }
    std::string last_error;
private:
    int level_;
};

class TextProfiler : public IProfiler {
public:
    void reportLayerTime(const char* name, float ms) override { rows.emplace_back(name, ms); }
    std::vector<std::pair<std::string, float>> rows;
};

int fail(const std::string& msg) {
    g_net_err = msg;
    return RT_E_BADARG;
}

// Device memory a net owns: freed with it, never copied.
struct DeviceBuffer {
    void* p = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { rt_free(p); }
    // made once, at the size its first use asks for
    bool ensure(size_t n) { return p || grow(n); }
    // replaced by a larger one when a call needs more (the old contents are not kept)
    bool grow(size_t n) {
        if (n <= bytes) return true;
        rt_free(p);
        p = nullptr;
        bytes = rt_malloc(&p, n) == 0 ? n : 0;
        if (!bytes) p = nullptr;                  // (whatever a failed allocation left there is not ours to free)
        return bytes != 0;
    }
};

}  // namespace

struct rtStereoNet {
    NetLogger log;
    std::vector<char> blob;                       // weight file image; Weights::values point into it
    weight_map weights;
    std::unique_ptr<IPluginContainer> plugins;
    ICudaEngine* engine = nullptr;
    IExecutionContext* context = nullptr;
    int layers = 0, width = 0, height = 0, max_batch = 1;
    int model = RT_MODEL_RESNET18_2D;
    // The frame path's buffers (run_frames), all for max_batch, none made before a call needs it.
    DeviceBuffer frame_in[2], frame_disp;         // the engine's three bindings: fp32 inputs and disparity, the same for every entry
    DeviceBuffer frame_px, frame_mask;            // RT_GEOM_FRAME: network-geometry pixels and mask
    DeviceBuffer points_ws;                       // compact clouds: rt_disparity_to_points' workspace, grown on demand
    DeviceBuffer rect[2];                         // raw frames without caller buffers: dense rectified frames, grown on demand
    DeviceBuffer color[2];                        // wire frames without caller buffers: dense decoded frames, grown on demand
    DeviceBuffer speckle_ws;                      // with a filter: rt_disparity_speckle's workspace
    DeviceBuffer voxel_cloud, voxel_ws;           // with a voxel grid: the organised cloud where the caller asks for none, and rt_points_voxel_grid's workspace; grown on demand
    ~rtStereoNet() {                              // (the buffers go after the engine that may still name them)
        if (context) context->destroy();
        if (engine) engine->destroy();
    }
};

namespace {

// name '\0' uint32 count, count elements (reference reader: sample_app/main.cpp:111-134)
bool parseWeights(rtStereoNet& n, int dtype) {
    const size_t el = dtype == RT_F16 ? 2 : 4;
    size_t off = 0;
    const std::vector<char>& b = n.blob;
    while (off < b.size()) {
        const void* z = memchr(b.data() + off, 0, b.size() - off);
        if (!z) return false;
        std::string name(b.data() + off);
        off += name.size() + 1;
        if (off + 4 > b.size()) return false;
        uint32_t count;
        memcpy(&count, b.data() + off, 4);
        off += 4;
        if (off + (size_t)count * el > b.size()) return false;
        if (n.weights.count(name)) return false;
        n.weights[name] = Weights{dtype == RT_F16 ? DataType::kHALF : DataType::kFLOAT, b.data() + off, (int64_t)count};
        off += (size_t)count * el;
    }
    return !n.weights.empty();
}

// what every execute entry binds: left, right, disp, in that order
bool bindings_ok(const ICudaEngine& e) {
    return e.getNbBindings() == 3 && e.getBindingIndex("left") == 0 && e.getBindingIndex("right") == 1 && e.getBindingIndex("disp") == 2;
}

int build(rtStereoNet** out, int model, int width, int height, int max_batch, int dtype, int max_disp,
          std::vector<char>&& blob, unsigned flags = 0) {
    if (!out) return fail("rt_net_create: null out pointer");
    if (width < 17 || height < 17 || max_batch < 1) return fail("rt_net_create: bad dimensions");
    if (dtype != RT_F32 && dtype != RT_F16) return fail("rt_net_create: weights_dtype must be RT_F32 or RT_F16");
    std::unique_ptr<rtStereoNet> n(new rtStereoNet());
    n->blob = std::move(blob);
    n->width = width; n->height = height; n->max_batch = max_batch; n->model = model;
    if (!parseWeights(*n, dtype)) return fail("rt_net_create: malformed weight file (expected name\\0, uint32 count, data ...)");
    n->plugins = IPluginContainer::create(n->log);
    IBuilder* builder = createInferBuilder(n->log);
    const DimsCHW dims{3, height, width};
    // The sample application keeps the plugins' DataType at kFLOAT for the 3-D models and passes its command-line data
    // type to the ResNet-18 2D builder (sample_app/main.cpp:228-256).  Here the plugin type stays kFLOAT for every model: what
    // an fp16 weight file switches on is half2 mode of the builder (fp16 storage between fused launches), and the executor
    // also accepts plugins created for kHALF as long as they are fused away (tests/test_sample_app.py drives that path)
    const DataType act_type = DataType::kFLOAT;
    INetworkDefinition* net = nullptr;
    switch (model) {
        case RT_MODEL_RESNET18_2D:
            net = createResNet18_2DNetwork(*builder, *n->plugins, dims, n->weights, act_type, max_disp > 0 ? max_disp : 48, n->log);
            break;
        case RT_MODEL_NVSMALL:
            net = createStereo3DNetwork(*builder, *n->plugins, Stereo3DModel::kNVSmall, dims, n->weights, act_type, max_disp > 0 ? max_disp : 48, n->log);
            break;
        case RT_MODEL_NVTINY:
            net = createStereo3DNetwork(*builder, *n->plugins, Stereo3DModel::kNVTiny, dims, n->weights, act_type, max_disp > 0 ? max_disp : 24, n->log);
            break;
        case RT_MODEL_RESNET18:
            net = createStereo3DNetwork(*builder, *n->plugins, Stereo3DModel::kResNet18, dims, n->weights, act_type, max_disp > 0 ? max_disp : 68, n->log);
            break;
        default:
            builder->destroy();
            return fail("rt_net_create: unknown model");
    }
    if (!net) {
        builder->destroy();
        return fail("rt_net_create: network construction failed: " + n->log.last_error);
    }
    n->layers = net->getNbLayers();
    builder->setMaxBatchSize(max_batch);
    builder->setHalf2Mode(dtype == RT_F16);        // fp16 weight file = fp16 inference, as in sample_app/main.cpp:256-262
    builder->setExactFp32Mode((flags & RT_CONV_EXACT_FP32) != 0);
    builder->setMaxWorkspaceSize((size_t)1 << 30);
    n->engine = builder->buildCudaEngine(*net);
    net->destroy();
    builder->destroy();
    if (!n->engine) return fail("rt_net_create: engine build failed: " + n->log.last_error);
    if (!bindings_ok(*n->engine)) return fail("rt_net_create: unexpected bindings");
    n->context = n->engine->createExecutionContext();
    if (!n->context) return fail("rt_net_create: context creation failed");
    *out = n.release();
    return 0;
}

// a weight file as it lies on the disk
int read_image(const std::string& fn, const char* path, std::vector<char>& image) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f.is_open()) return fail(fn + "cannot open " + path);
    image.resize((size_t)f.tellg());
    f.seekg(0);
    f.read(image.data(), (std::streamsize)image.size());
    return 0;
}

// The weight image travels root -> everyone over RCCL: its size first, then its bytes.  comm == NULL is a world of one.
int broadcast_image(const std::string& fn, rtComm* comm, int root, std::vector<char>& image) {
    int world = 1, rank = 0;
    if (comm && rt_comm_info(comm, &world, &rank) != 0) return fail(fn + rt_last_error_string());
    if (root < 0 || root >= world) return fail(fn + "root is not a rank of the communicator");
    if (rank == root && image.empty()) return fail(fn + "the root rank has no weight image");
    uint64_t n = rank == root ? (uint64_t)image.size() : 0;
    if (comm && rt_comm_broadcast(comm, &n, sizeof(n), root, nullptr) != 0) return fail(fn + rt_last_error_string());
    if (n == 0 || n > ((uint64_t)1 << 32)) return fail(fn + "implausible weight image size received");
    image.resize((size_t)n);
    if (comm && rt_comm_broadcast(comm, image.data(), (size_t)n, root, nullptr) != 0) return fail(fn + rt_last_error_string());
    return 0;
}

}  // namespace

extern "C" const char* rt_net_last_error(void) { return g_net_err.c_str(); }

extern "C" int rt_net_create(rtStereoNet** net, int model, int width, int height, int max_batch, int dtype, int max_disp,
                             const char* path) {
    if (!path) return fail("rt_net_create: null weights path");
    std::vector<char> image;
    if (read_image("rt_net_create: ", path, image) != 0) return RT_E_BADARG;
    return build(net, model, width, height, max_batch, dtype, max_disp, std::move(image));
}

extern "C" int rt_net_create_from_memory(rtStereoNet** net, int model, int width, int height, int max_batch, int dtype,
                                         int max_disp, const void* blob, size_t bytes) {
    if (!blob || !bytes) return fail("rt_net_create_from_memory: empty blob");
    std::vector<char> copy(static_cast<const char*>(blob), static_cast<const char*>(blob) + bytes);
    return build(net, model, width, height, max_batch, dtype, max_disp, std::move(copy));
}

// Multi-GPU start-up (include/rt_stereo_net.h): the weight image travels root -> everyone over RCCL, then every rank builds its engine.
extern "C" int rt_net_create_broadcast(rtStereoNet** net, int model, int width, int height, int max_batch, int dtype, int max_disp,
                                       const void* blob, size_t bytes, rtComm* comm, int root) {
    std::vector<char> image;
    if (blob && bytes) image.assign(static_cast<const char*>(blob), static_cast<const char*>(blob) + bytes);
    if (broadcast_image("rt_net_create_broadcast: ", comm, root, image) != 0) return RT_E_BADARG;
    return build(net, model, width, height, max_batch, dtype, max_disp, std::move(image));
}

extern "C" int rt_net_create_opt(rtStereoNet** net, const rtNetOptions* o) {
    if (!o) return fail("rt_net_create_opt: null options");
    std::vector<char> image;
    if (o->weights_path && !o->blob) {
        if (read_image("rt_net_create_opt: ", o->weights_path, image) != 0) return RT_E_BADARG;
    } else if (o->blob && o->bytes) {
        image.assign(static_cast<const char*>(o->blob), static_cast<const char*>(o->blob) + o->bytes);
    }
    if (o->comm && broadcast_image("rt_net_create_opt: ", o->comm, o->root, image) != 0) return RT_E_BADARG;
    if (image.empty()) return fail("rt_net_create_opt: no weights (weights_path, blob or a broadcast)");
    return build(net, o->model, o->width, o->height, o->max_batch, o->weights_dtype, o->max_disp, std::move(image), o->flags);
}

extern "C" int rt_net_set_debug(rtStereoNet* net, int on) {
    if (!net || !net->context) return fail("rt_net_set_debug: null pointer");
    net->context->setDebugSync(on != 0);
    return 0;
}

extern "C" int rt_net_weights_crc32(const rtStereoNet* net, uint32_t* crc) {
    if (!net || !crc) return fail("rt_net_weights_crc32: null pointer");
    uint32_t c = 0xffffffffu;
    for (unsigned char b : net->blob) {
        c ^= b;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    *crc = c ^ 0xffffffffu;
    return 0;
}

extern "C" int rt_net_weights_image(const rtStereoNet* net, const void** data, size_t* bytes) {
    if (!net || !data || !bytes) return fail("rt_net_weights_image: null pointer");
    *data = net->blob.data();
    *bytes = net->blob.size();
    return 0;
}

// Engine plan = what ICudaEngine::serialize() returns (sample_app/main.cpp:269-275 caches it in a .plan file).
// Call with buf == NULL to query the size.  Networks with non-serialisable plugins (the 3-D models) have no plan,
// exactly as in the reference.
extern "C" int rt_net_serialize(rtStereoNet* net, void* buf, size_t buf_bytes, size_t* plan_bytes) {
    if (!net || !plan_bytes) return fail("rt_net_serialize: null pointer");
    IHostMemory* m = net->engine->serialize();
    if (!m) return fail("rt_net_serialize: " + net->log.last_error);
    *plan_bytes = m->size();
    int rc = 0;
    if (buf) {
        if (buf_bytes < m->size()) rc = fail("rt_net_serialize: buffer too small");
        else memcpy(buf, m->data(), m->size());
    }
    m->destroy();
    return rc;
}

// Counterpart of sample_app/main.cpp:198-220: IRuntime::deserializeCudaEngine(plan, size, &StereoDnnPluginFactory).
extern "C" int rt_net_create_from_plan(rtStereoNet** out, const void* plan, size_t plan_bytes) {
    if (!out || !plan || !plan_bytes) return fail("rt_net_create_from_plan: null pointer");
    std::unique_ptr<rtStereoNet> n(new rtStereoNet());
    n->plugins = IPluginContainer::create(n->log);
    StereoDnnPluginFactory factory(*n->plugins);
    IRuntime* runtime = createInferRuntime(n->log);
    n->engine = runtime->deserializeCudaEngine(plan, plan_bytes, &factory);
    runtime->destroy();
    if (!n->engine) return fail("rt_net_create_from_plan: " + n->log.last_error);
    if (!bindings_ok(*n->engine)) return fail("rt_net_create_from_plan: unexpected bindings");
    n->max_batch = n->engine->getMaxBatchSize();
    // a plan knows its input size; only ResNet-18 2D has one (rt_net_serialize fails for the 3-D models' plugins)
    const Dims in = n->engine->getBindingDimensions(0);
    if (in.nbDims != 3 || in.d[0] != 3 || in.d[1] < 1 || in.d[2] < 1) return fail("rt_net_create_from_plan: unexpected input binding");
    n->height = in.d[1];
    n->width = in.d[2];
    n->model = RT_MODEL_RESNET18_2D;
    n->context = n->engine->createExecutionContext();
    if (!n->context) return fail("rt_net_create_from_plan: context creation failed");
    *out = n.release();
    return 0;
}

extern "C" int rt_net_execute(rtStereoNet* net, const void* left, const void* right, void* disp, int batch, rtStream stream) {
    if (!net || !left || !right || !disp) return fail("rt_net_execute: null pointer");
    void* bindings[3] = {const_cast<void*>(left), const_cast<void*>(right), disp};
    const bool ok = stream ? net->context->enqueue(batch, bindings, (cudaStream_t)stream, nullptr) : net->context->execute(batch, bindings);
    if (!ok) return fail("rt_net_execute: " + net->log.last_error);
    return 0;
}

// ---- the camera-frame path ---------------------------------------------------------------------------------------------------------------
// The nine rt_net_execute_frames* entries fill a FrameJob and make the checks that are theirs alone; run_frames does everything else, once:
//   validate everything -> make or grow the net's buffers -> [rt_rectify_frames_u8] -> rt_preprocess_frames_u8 / _u8_lr / _u8_cv
//   -> one engine pass at batch (2 * batch with a check) on the net's three bindings
//   -> [rt_lr_consistency | rt_disparity_scale] -> [rt_disparity_speckle]
//   -> one back end: network geometry (copy, scale or 16-bit; with a check rt_lr_consistency is the back end), rt_disparity_to_frame or
//      rt_disparity_to_points -> [rt_points_voxel_grid]
//   -> [rt_viz_mosaic_u8] -> one rt_stream_sync when there is no stream.
// It is the ROS node's computeOutputs (stereo_dnn_ros_node.cpp:60-103) after the H2D copy of the raw frames, the sample app's result path
// (sample_app/main.cpp:321-330) and the viz node's panel (stereo_dnn_ros_viz_node.cpp:81-130), on the device.  Whatever an op-level call
// can refuse is refused before anything is written: by the checks here, which precede the decode and the rectify launch, or by the front
// end, whose limits are the back end's.
namespace {

struct FrameJob {
    const rtFrameCall* c = nullptr;                // frames and their geometry, resize, output geometry, disparity and its kind, check, batch
    bool need_check = false;                       // rt_net_execute_frames_lr: a tolerance is not optional
    void* disp_right = nullptr;                    // ... and the right view's disparity comes out
    const rtDepthCall* d = nullptr;                // rt_disparity_to_points in the place of rt_disparity_to_frame; c->disp optional
    const rtRectifyCall* r = nullptr;              // c's frames are raw: everything else runs on their rectified form
    const rtSpeckleCall* sp = nullptr;             // rt_disparity_speckle in network geometry; the back end then always gets a mask
    const rtDecodeCall* dec = nullptr;             // c's frames are wire frames (mono, Bayer, YUV 4:2:2): everything else runs on their decoded form
    const rtVoxelCall* vx = nullptr;               // rt_points_voxel_grid behind rt_disparity_to_points; d required, its outputs optional
    void* viz_rgb8 = nullptr;                      // the viz node's panel of c's frames and c->disp
    int64_t viz_step = 0;
    float max_disp = 0.f;
};

int run_frames(const std::string& fn, rtStereoNet* net, const FrameJob& j, rtStream stream) {
    const rtFrameCall* c = j.c;
    const rtDepthCall* d = j.d;
    const rtRectifyCall* r = j.r;
    const rtSpeckleCall* sp = j.sp;
    const rtDecodeCall* dec = j.dec;
    const rtVoxelCall* vx = j.vx;
    if (!net || !net->context || !c || (vx && !d)) return fail(fn + "null pointer");
    const auto wrong_size = [&fn](size_t got, size_t want, const char* type) {
        return fail(fn + "struct_bytes " + std::to_string(got) + " is not sizeof(" + type + ") = " + std::to_string(want));
    };
    if (r && r->struct_bytes != sizeof(rtRectifyCall)) return wrong_size(r->struct_bytes, sizeof(rtRectifyCall), "rtRectifyCall");
    if (c->struct_bytes != sizeof(rtFrameCall)) return wrong_size(c->struct_bytes, sizeof(rtFrameCall), "rtFrameCall");
    if (d && d->struct_bytes != sizeof(rtDepthCall)) return wrong_size(d->struct_bytes, sizeof(rtDepthCall), "rtDepthCall");
    if (sp && sp->struct_bytes != sizeof(rtSpeckleCall)) return wrong_size(sp->struct_bytes, sizeof(rtSpeckleCall), "rtSpeckleCall");
    if (dec && dec->struct_bytes != sizeof(rtDecodeCall)) return wrong_size(dec->struct_bytes, sizeof(rtDecodeCall), "rtDecodeCall");
    if (vx && vx->struct_bytes != sizeof(rtVoxelCall)) return wrong_size(vx->struct_bytes, sizeof(rtVoxelCall), "rtVoxelCall");
    if (!c->left_u8 || !c->right_u8 || (!d && !c->disp)) return fail(fn + "null pointer");
    if (c->resize != RT_RESIZE_AREA_DOWN && c->resize != RT_RESIZE_CV_AREA) return fail(fn + "unknown resize " + std::to_string(c->resize));
    if (c->geometry != RT_GEOM_NET && c->geometry != RT_GEOM_FRAME) return fail(fn + "unknown geometry " + std::to_string(c->geometry));
    if ((!d || c->disp) && c->disp_kind != RT_DISP_NET && c->disp_kind != RT_DISP_PIXELS_F32 && c->disp_kind != RT_DISP_KITTI_U16)
        return fail(fn + "unknown disp_kind " + std::to_string(c->disp_kind));
    if (d) {                                           // what only rt_disparity_to_points can refuse
        constexpr float kMax = 3.402823466e38f;
        const rtStereoCamera& k = d->camera;
        if (c->geometry != RT_GEOM_FRAME) {
            fail(fn + "depth and cloud exist in the camera's own geometry only: RT_GEOM_NET is not supported, use RT_GEOM_FRAME");
            return RT_E_UNSUPPORTED;
        }
        if (!d->depth && !d->points && !d->points_compact && !d->count && !c->disp && !vx) return fail(fn + "no output requested");
        if (d->depth && d->depth_kind != RT_DEPTH_M_F32 && d->depth_kind != RT_DEPTH_MM_U16)
            return fail(fn + "unknown depth_kind " + std::to_string(d->depth_kind));
        if (!(k.fx > 0.f && k.fx <= kMax && k.fy > 0.f && k.fy <= kMax && k.baseline > 0.f && k.baseline <= kMax))
            return fail(fn + "fx, fy and baseline must be finite numbers > 0");
        if (!(std::fabs(k.cx) <= kMax && std::fabs(k.cy) <= kMax && std::fabs(k.doffs) <= kMax)) return fail(fn + "cx, cy and doffs must be finite");
        if (!(d->min_depth >= 0.f)) return fail(fn + "min_depth must be a number >= 0");
        if (!(d->max_depth >= d->min_depth)) return fail(fn + "max_depth must be a number >= min_depth");
        if (d->points_compact && !d->count) return fail(fn + "points_compact needs count");
        if (((reinterpret_cast<uintptr_t>(d->points) | reinterpret_cast<uintptr_t>(d->points_compact)) & 15) != 0)
            return fail(fn + "a cloud must start on a 16-byte boundary");
    }
    if (sp) {                                          // what only rt_disparity_speckle can refuse
        if (c->geometry != RT_GEOM_FRAME) {
            fail(fn + "the speckle filter runs in front of the resampling to the frame: RT_GEOM_NET is not supported, use RT_GEOM_FRAME");
            return RT_E_UNSUPPORTED;
        }
        if (sp->max_size < 0) return fail(fn + "speckle max_size must be >= 0");
        if (!(sp->max_diff_px >= 0.f && sp->max_diff_px <= 3.402823466e38f)) return fail(fn + "speckle max_diff_px must be a finite number >= 0");
    }
    if (c->encoding < RT_ENC_BGR8 || c->encoding > RT_ENC_RGBA8) return fail(fn + "unknown encoding " + std::to_string(c->encoding));
    if (j.need_check && !(c->max_diff_px >= 0.f)) return fail(fn + "max_diff_px must be a number >= 0");
    if (c->max_diff_px != c->max_diff_px) return fail(fn + "max_diff_px is not a number");
    const bool check = c->max_diff_px >= 0.f;
    if (!check && !sp && (c->mask_u8 || c->valid_count)) return fail(fn + "mask_u8 and valid_count need a check (max_diff_px >= 0)");
    const int batch = c->batch, engine_batch = check ? 2 * batch : batch;
    if (batch < 1 || (int64_t)(check ? 2 : 1) * batch > net->max_batch)
        return fail(fn + "batch " + std::to_string(batch) + (check ? " with a check" : "") + " needs an engine batch of " +
                    std::to_string((int64_t)(check ? 2 : 1) * batch) + ", max_batch is " + std::to_string(net->max_batch));
    const bool frame = c->geometry == RT_GEOM_FRAME;   // (with d or sp: always)
    if (frame && (!d || c->disp) && c->disp_kind == RT_DISP_NET) {
        fail(fn + "RT_GEOM_FRAME needs a disparity in pixels (RT_DISP_PIXELS_F32 / RT_DISP_KITTI_U16), not RT_DISP_NET");
        return RT_E_UNSUPPORTED;
    }
    if (vx) {                                          // what only rt_points_voxel_grid can refuse
        if (!vx->voxels || !vx->count) return fail(fn + "null pointer");
        if (c->src_h < 1 || c->src_w < 1) return fail(fn + "bad dims");
        const int64_t records = (int64_t)c->src_h * c->src_w;
        if (records > (1 << 23)) return fail(fn + "a frame of more than 2^23 pixels is beyond the voxel grid's limits");
        if (vx->capacity < 1 || vx->capacity > (1 << 23)) return fail(fn + "voxel capacity " + std::to_string(vx->capacity) + " outside [1, 2^23]");
        if (vx->min_points < 1) return fail(fn + "min_points must be >= 1");
        if ((reinterpret_cast<uintptr_t>(vx->voxels) & 15) != 0) return fail(fn + "a cloud must start on a 16-byte boundary");
        if ((reinterpret_cast<uintptr_t>(vx->count) & 7) != 0 || ((reinterpret_cast<uintptr_t>(vx->cell_u32) | reinterpret_cast<uintptr_t>(vx->n_u32)) & 3) != 0)
            return fail(fn + "voxel count must start on an 8-byte boundary, cell_u32 and n_u32 on a 4-byte boundary");
        if (rt_voxel_workspace_bytes(batch, (int)records, &vx->grid) == 0)
            return fail(fn + "the batch or the grid is beyond rt_points_voxel_grid's limits (dims in [1, 4096], at most 2^27 cells, leaf finite and > 0, "
                             "origin finite)");
        struct Range { const void* p; size_t n; };
        const size_t nb = (size_t)batch;
        const Range outs[4] = {{vx->voxels, nb * vx->capacity * 16}, {vx->count, nb * 8}, {vx->cell_u32, nb * vx->capacity * 4}, {vx->n_u32, nb * vx->capacity * 4}};
        const Range ins[2] = {{d->points ? d->points : d->points_compact, nb * (size_t)records * 16}, {d->points ? nullptr : d->count, nb * 8}};
        const auto overlap = [](const Range& a, const Range& b) {
            const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
            return a.p && b.p && x < y + b.n && y < x + a.n;
        };
        for (int i = 0; i < 4; i++) {
            for (const Range& in : ins)
                if (overlap(outs[i], in)) return fail(fn + "a voxel output overlaps the cloud it is made from");
            for (int k = i + 1; k < 4; k++)
                if (overlap(outs[i], outs[k])) return fail(fn + "two voxel outputs overlap");
        }
    }
    const int H = net->height, W = net->width;
    const int bpp = c->encoding == RT_ENC_BGRA8 || c->encoding == RT_ENC_RGBA8 ? 4 : 3;
    rtFrameCall decoded, rectified;
    if (r || dec) {
        // What the front end, rt_decode_frames_u8 and rt_rectify_frames_u8 would refuse, found here: behind the first of these launches an
        // error could no longer write nothing.  The frames the caller passes are wire frames with `dec`, and their step is held against
        // the wire pixel.
        if (dec && (dec->wire_encoding < RT_WIRE_MONO8 || dec->wire_encoding > RT_WIRE_YUV422_YUY2))
            return fail(fn + "unknown wire encoding " + std::to_string(dec->wire_encoding));
        const int in_bpp = !dec ? bpp : dec->wire_encoding == RT_WIRE_MONO16 || dec->wire_encoding >= RT_WIRE_YUV422 ? 2 : 1;
        if (c->src_h < 1 || c->src_w < 1 || c->src_h > (1 << 24) || c->src_w > (1 << 24) || (int64_t)c->src_h * c->src_w >= ((int64_t)1 << 31) ||
            batch > 32767)
            return fail(fn + "bad dims");
        if (c->src_step < (int64_t)c->src_w * in_bpp)
            return fail(fn + "row step " + std::to_string(c->src_step) + " is shorter than " + std::to_string(c->src_w) + " pixels of " +
                        std::to_string(in_bpp) + " bytes");
        const bool down = H <= c->src_h && W <= c->src_w;
        if (c->resize == RT_RESIZE_AREA_DOWN && !down)
            return fail(fn + "INTER_AREA up-scaling (" + std::to_string(c->src_w) + "x" + std::to_string(c->src_h) + " -> " + std::to_string(W) + "x" +
                        std::to_string(H) + ") is not implemented by RT_RESIZE_AREA_DOWN");
        if ((float)c->src_w / W > 6.f || (float)c->src_h / H > 6.f || (float)W / c->src_w > 6.f || (float)H / c->src_h > 6.f)
            return fail(fn + "scale factors outside [1/6, 6] are not implemented");
    }
    const size_t dense = (size_t)net->max_batch * c->src_h * c->src_w * bpp;      // frames of the net's own, decoded or rectified
    if (dec) {
        if (!dec->left_color_u8 != !dec->right_color_u8) return fail(fn + "left_color_u8 and right_color_u8: both or neither");
        if (dec->left_color_u8 ? dec->color_step < (int64_t)c->src_w * bpp : dec->color_step != 0)
            return fail(fn + "color_step " + std::to_string(dec->color_step) + (dec->left_color_u8 ? " is shorter than a row" : " without buffers"));
        if (dec->left_color_u8) {
            for (const void* p : {dec->left_color_u8, dec->right_color_u8}) {
                if (p == c->left_u8 || p == c->right_u8) return fail(fn + "a colour buffer must not be a wire buffer");
                if (r && (p == r->left_rect_u8 || p == r->right_rect_u8)) return fail(fn + "a colour buffer must not be a rectified buffer");
            }
        }
        decoded = *c;
        if (dec->left_color_u8) {
            decoded.left_u8 = dec->left_color_u8;
            decoded.right_u8 = dec->right_color_u8;
            decoded.src_step = dec->color_step;
        } else {
            if (!net->color[0].grow(dense) || !net->color[1].grow(dense)) return fail(fn + rt_last_error_string());
            decoded.left_u8 = net->color[0].p;
            decoded.right_u8 = net->color[1].p;
            decoded.src_step = (int64_t)c->src_w * bpp;
        }
    }
    if (r) {
        const rtFrameCall* raw = dec ? &decoded : c;       // what the rectify launch reads
        if (!r->left_rect_u8 != !r->right_rect_u8) return fail(fn + "left_rect_u8 and right_rect_u8: both or neither");
        if (r->left_rect_u8 ? r->rect_step < (int64_t)c->src_w * bpp : r->rect_step != 0)
            return fail(fn + "rect_step " + std::to_string(r->rect_step) + (r->left_rect_u8 ? " is shorter than a row" : " without buffers"));
        for (const rtRectifyCamera* k : {&r->left, &r->right}) {
            const double* v = reinterpret_cast<const double*>(k);
            for (size_t i = 0; i < sizeof(rtRectifyCamera) / sizeof(double); i++)
                if (!std::isfinite(v[i])) return fail(fn + "every field of a camera must be finite");
        }
        if (r->left_rect_u8 == raw->left_u8 || r->right_rect_u8 == raw->right_u8) return fail(fn + "a rectified buffer must not be the raw one");
        rectified = *raw;
        if (r->left_rect_u8) {
            rectified.left_u8 = r->left_rect_u8;
            rectified.right_u8 = r->right_rect_u8;
            rectified.src_step = r->rect_step;
        } else {
            if (!net->rect[0].grow(dense) || !net->rect[1].grow(dense)) return fail(fn + rt_last_error_string());
            rectified.left_u8 = net->rect[0].p;
            rectified.right_u8 = net->rect[1].p;
            rectified.src_step = (int64_t)c->src_w * bpp;
        }
    }
    if (dec) {                                             // the first launch: whatever it refuses, nothing has been written
        if (rt_decode_frames_u8(c->left_u8, c->right_u8, c->src_h, c->src_w, c->src_step, dec->wire_encoding, const_cast<void*>(decoded.left_u8),
                                const_cast<void*>(decoded.right_u8), decoded.src_step, c->encoding, batch, stream) != 0)
            return fail(fn + rt_last_error_string());
        c = &decoded;
    }
    if (r) {
        if (rt_rectify_frames_u8(c->left_u8, c->right_u8, c->src_h, c->src_w, c->src_step, c->encoding, &r->left, &r->right,
                                 const_cast<void*>(rectified.left_u8), const_cast<void*>(rectified.right_u8), c->src_h, c->src_w, rectified.src_step,
                                 batch, stream) != 0)
            return fail(fn + rt_last_error_string());
        c = &rectified;
    }
    // RT_RESIZE_AREA_DOWN into RT_GEOM_NET is what rt_net_execute_frames / _lr do, whichever entry asks: from here on an error reports
    // under their names (a front end's refusal reads the same through every entry)
    const std::string as = d || dec || c->resize != RT_RESIZE_AREA_DOWN || frame ? fn : check ? "rt_net_execute_frames_lr: " : "rt_net_execute_frames: ";
    const int64_t pixels = (int64_t)H * W;
    const size_t plane = (size_t)net->max_batch * pixels;
    if (!net->frame_in[0].ensure(3 * plane * sizeof(float)) || !net->frame_in[1].ensure(3 * plane * sizeof(float)) ||
        !net->frame_disp.ensure(plane * sizeof(float)))
        return fail(as + rt_last_error_string());
    if (frame && (!net->frame_px.ensure(plane * sizeof(float)) || !net->frame_mask.ensure(plane))) return fail(as + rt_last_error_string());
    // (rt_points_workspace_bytes is 0 for sizes the front end refuses below)
    if (d && (d->points_compact || d->count) && !net->points_ws.grow(rt_points_workspace_bytes(net->max_batch, c->src_h, c->src_w)))
        return fail(as + rt_last_error_string());
    if (vx) {
        const size_t records = (size_t)c->src_h * c->src_w;
        if (!d->points && !d->points_compact && !net->voxel_cloud.grow((size_t)batch * records * 16)) return fail(as + rt_last_error_string());
        if (!net->voxel_ws.grow(rt_voxel_workspace_bytes(batch, (int)records, &vx->grid))) return fail(as + rt_last_error_string());
    }
    if (sp && !net->speckle_ws.p) {
        const size_t need = rt_speckle_workspace_bytes(net->max_batch, H, W);
        if (need == 0) return fail(as + "the network's size is beyond the speckle filter's limits");
        if (!net->speckle_ws.ensure(need)) return fail(as + rt_last_error_string());
    }
    // (argument errors of the pre-processing -- short step, up-scaling, factors above 6 -- are found before anything is written)
    int rc;
    if (c->resize == RT_RESIZE_CV_AREA)
        rc = rt_preprocess_frames_u8_cv(c->left_u8, c->right_u8, c->src_h, c->src_w, c->src_step, c->encoding, net->frame_in[0].p, net->frame_in[1].p, H,
                                        W, batch, check ? 1 : 0, stream);
    else
        rc = (check ? rt_preprocess_frames_u8_lr : rt_preprocess_frames_u8)(c->left_u8, c->right_u8, c->src_h, c->src_w, c->src_step, c->encoding,
                                                                            net->frame_in[0].p, net->frame_in[1].p, H, W, batch, stream);
    if (rc != 0) return fail(as + rt_last_error_string());
    // The same three bindings for every entry (sized for max_batch, and 2 * batch <= max_batch with a check), so the engine's graph for
    // batch 2b lives beside the one for batch b.
    void* bindings[3] = {net->frame_in[0].p, net->frame_in[1].p, net->frame_disp.p};
    const bool ok = stream ? net->context->enqueue(engine_batch, bindings, (cudaStream_t)stream, nullptr) : net->context->execute(engine_batch, bindings);
    if (!ok) return fail(as + net->log.last_error);
    // ResNet-18 2D's sigmoid output is disparity / width; the 3-D models' soft-argmin is in pixels (sample_app/main.cpp:325-327)
    const float scale = net->model == RT_MODEL_RESNET18_2D ? (float)W : 1.f;
    const int64_t n = batch * pixels;
    if (!frame) {
        if (check) rc = rt_lr_consistency(net->frame_disp.p, batch, H, W, scale, c->max_diff_px, c->disp, c->disp_kind, c->mask_u8, j.disp_right, c->valid_count, stream);
        else if (c->disp_kind == RT_DISP_NET) rc = rt_memcpy_d2d(c->disp, net->frame_disp.p, (size_t)n * sizeof(float), stream);
        else if (c->disp_kind == RT_DISP_PIXELS_F32) rc = rt_disparity_scale(net->frame_disp.p, c->disp, n, scale, stream);
        else rc = rt_disparity_to_u16(net->frame_disp.p, c->disp, n, 256.f * scale, stream);
    } else {
        const void* px = net->frame_disp.p;            // the 3-D models' output is in pixels already
        const void* mask = nullptr;
        if (check) {
            rc = rt_lr_consistency(net->frame_disp.p, batch, H, W, scale, c->max_diff_px, net->frame_px.p, RT_DISP_PIXELS_F32, net->frame_mask.p, nullptr, nullptr, stream);
            px = net->frame_px.p;
            mask = net->frame_mask.p;
        } else if (net->model == RT_MODEL_RESNET18_2D) {
            rc = rt_disparity_scale(net->frame_disp.p, net->frame_px.p, n, scale, stream);
            px = net->frame_px.p;
        }
        if (rc == 0 && sp) {                           // in place on frame_px / frame_mask, or out of place from frame_disp where no step ran
            rc = rt_disparity_speckle(px, mask, batch, H, W, sp->max_size, sp->max_diff_px, net->frame_px.p, net->frame_mask.p, nullptr, net->speckle_ws.p,
                                      net->speckle_ws.bytes, stream);
            px = net->frame_px.p;
            mask = net->frame_mask.p;
        }
        // (without a mask c->mask_u8 and c->valid_count are NULL: checked above)
        if (rc == 0 && d) {
            // the cloud the voxel grid is made from: the caller's organised one, else the caller's compact one, else the net's own (organised)
            void* organised = d->points || !vx || d->points_compact ? d->points : net->voxel_cloud.p;
            rc = rt_disparity_to_points(px, mask, batch, H, W, c->src_h, c->src_w, &d->camera, d->min_depth, d->max_depth, c->left_u8, c->src_step,
                                        c->encoding, c->disp, c->disp_kind, c->mask_u8, c->valid_count, d->depth, d->depth_kind, organised,
                                        d->points_compact, d->count, net->points_ws.p, net->points_ws.bytes, stream);
            if (rc == 0 && vx)
                rc = rt_points_voxel_grid(organised ? organised : d->points_compact, organised ? nullptr : d->count, batch, c->src_h * c->src_w, &vx->grid,
                                          vx->min_points, vx->voxels, vx->capacity, vx->count, vx->cell_u32, vx->n_u32, net->voxel_ws.p,
                                          net->voxel_ws.bytes, stream);
        } else if (rc == 0)
            rc = rt_disparity_to_frame(px, mask, batch, H, W, c->disp, c->disp_kind, c->src_h, c->src_w, c->mask_u8, c->valid_count, stream);
    }
    if (rc != 0) return fail(as + rt_last_error_string());
    if (j.viz_rgb8)
        rc = rt_viz_mosaic_u8(c->left_u8, c->right_u8, c->src_h, c->src_w, c->src_step, c->encoding, c->disp, H, W, j.max_disp, j.viz_rgb8, j.viz_step,
                              batch, stream);
    if (rc == 0 && !stream) rc = rt_stream_sync(nullptr);
    if (rc != 0) return fail((j.viz_rgb8 ? "rt_net_execute_frames_viz: " : as) + rt_last_error_string());
    return 0;
}

// rt_net_execute_frames (need_check off) and rt_net_execute_frames_lr (on), and rt_net_execute_frames_viz behind its own checks: flat
// arguments, RT_RESIZE_AREA_DOWN into RT_GEOM_NET, and their own words for a batch that does not fit.
int run_flat(rtStereoNet* net, const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step, int encoding, void* disp,
             int disp_kind, float max_diff_px, void* mask_u8, void* valid_count, int batch, FrameJob j, rtStream stream) {
    const std::string fn = j.need_check ? "rt_net_execute_frames_lr: " : "rt_net_execute_frames: ";
    if (!net || !net->context || !left_u8 || !right_u8 || !disp) return fail(fn + "null pointer");
    if (batch < 1 || (int64_t)(j.need_check ? 2 : 1) * batch > net->max_batch)
        return fail(fn + "batch " + std::to_string(batch) +
                    (j.need_check ? " needs an engine batch of " + std::to_string(2 * (int64_t)batch) + ", max_batch is " : " outside 1..") +
                    std::to_string(net->max_batch));
    const rtFrameCall c = {sizeof(rtFrameCall), left_u8, right_u8, src_h, src_w, src_step, encoding, RT_RESIZE_AREA_DOWN, disp, disp_kind, RT_GEOM_NET,
                           max_diff_px, mask_u8, valid_count, batch};
    j.c = &c;
    return run_frames(fn, net, j, stream);
}

// the four entries that take an rtFrameCall: each optional part that is absent leaves the entry below it, which also gives the call its name
int run_call(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out, const rtRectifyCall* rect, const rtSpeckleCall* speckle,
             rtStream stream) {
    FrameJob j;
    j.c = call;
    j.d = out;
    j.r = rect;
    j.sp = speckle;
    return run_frames(speckle ? "rt_net_execute_frames_filtered: " : rect ? "rt_net_execute_frames_raw: " : out ? "rt_net_execute_frames_3d: "
                                                                                                                : "rt_net_execute_frames_ex: ",
                      net, j, stream);
}

}  // namespace

extern "C" int rt_net_execute_frames(rtStereoNet* net, const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step,
                                     int encoding, void* disp, int disp_kind, int batch, rtStream stream) {
    return run_flat(net, left_u8, right_u8, src_h, src_w, src_step, encoding, disp, disp_kind, -1.f, nullptr, nullptr, batch, FrameJob(), stream);
}

// rt_net_execute_frames with a left-right consistency check: the mirrored, swapped pair rides as the second half of one engine batch.
extern "C" int rt_net_execute_frames_lr(rtStereoNet* net, const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step,
                                        int encoding, void* disp, int disp_kind, void* mask_u8, void* disp_right, void* valid_count,
                                        float max_diff_px, int batch, rtStream stream) {
    FrameJob j;
    j.need_check = true;
    j.disp_right = disp_right;
    return run_flat(net, left_u8, right_u8, src_h, src_w, src_step, encoding, disp, disp_kind, max_diff_px, mask_u8, valid_count, batch, j, stream);
}

// The DNN node's disparity and the viz node's panel from one call.  What only the panel can refuse is checked first, so that an error
// writes nothing; everything else is refused as rt_net_execute_frames / _lr refuse it.
extern "C" int rt_net_execute_frames_viz(rtStereoNet* net, const void* left_u8, const void* right_u8, int src_h, int src_w, int64_t src_step,
                                         int encoding, void* disp_px, void* viz_rgb8, int64_t viz_step, float max_disp, float max_diff_px,
                                         void* mask_u8, void* valid_count, int batch, rtStream stream) {
    if (!net || !net->context || !left_u8 || !right_u8 || !disp_px || !viz_rgb8) return fail("rt_net_execute_frames_viz: null pointer");
    if (!(max_disp > 0.f && max_disp <= 3.402823466e38f)) return fail("rt_net_execute_frames_viz: max_disp must be a number > 0");
    if (viz_step < 6 * (int64_t)net->width)
        return fail("rt_net_execute_frames_viz: viz_step " + std::to_string(viz_step) + " is shorter than " + std::to_string(2 * net->width) +
                    " pixels of 3 bytes");
    if (max_diff_px != max_diff_px) return fail("rt_net_execute_frames_viz: max_diff_px is not a number");
    const bool check = max_diff_px >= 0.f;
    if (!check && (mask_u8 || valid_count)) return fail("rt_net_execute_frames_viz: mask_u8 and valid_count need a check (max_diff_px >= 0)");
    FrameJob j;
    j.need_check = check;
    j.viz_rgb8 = viz_rgb8;
    j.viz_step = viz_step;
    j.max_disp = max_disp;
    return run_flat(net, left_u8, right_u8, src_h, src_w, src_step, encoding, disp_px, RT_DISP_PIXELS_F32, check ? max_diff_px : -1.f, mask_u8,
                    valid_count, batch, j, stream);
}

// Frames of any size in, disparity in the network's or in the frame's geometry out.
extern "C" int rt_net_execute_frames_ex(rtStereoNet* net, const rtFrameCall* call, rtStream stream) {
    return run_call(net, call, nullptr, nullptr, nullptr, stream);
}

// ... in frame geometry with depth and / or a point cloud beside (or instead of) the disparity
extern "C" int rt_net_execute_frames_3d(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out, rtStream stream) {
    return run_call(net, call, out, nullptr, nullptr, stream);
}

// ... from raw frames: one rt_rectify_frames_u8 launch in front, everything else on its output
extern "C" int rt_net_execute_frames_raw(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out, const rtRectifyCall* rect,
                                         rtStream stream) {
    if (!rect) return fail("rt_net_execute_frames_raw: null pointer");
    return run_call(net, call, out, rect, nullptr, stream);
}

// ... with a speckle filter in network geometry, in front of the resampling
extern "C" int rt_net_execute_frames_filtered(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out, const rtRectifyCall* rect,
                                              const rtSpeckleCall* speckle, rtStream stream) {
    return run_call(net, call, out, rect, speckle, stream);
}

// ... from what the camera really sends: one rt_decode_frames_u8 launch in front, everything else on its output
extern "C" int rt_net_execute_frames_camera(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out, const rtRectifyCall* rect,
                                            const rtSpeckleCall* speckle, const rtDecodeCall* decode, rtStream stream) {
    if (!decode) return run_call(net, call, out, rect, speckle, stream);
    FrameJob j;
    j.c = call;
    j.d = out;
    j.r = rect;
    j.sp = speckle;
    j.dec = decode;
    return run_frames("rt_net_execute_frames_camera: ", net, j, stream);
}

// ... with the cloud put on a voxel grid: one rt_points_voxel_grid behind rt_disparity_to_points
extern "C" int rt_net_execute_frames_voxels(rtStereoNet* net, const rtFrameCall* call, const rtDepthCall* out, const rtRectifyCall* rect,
                                            const rtSpeckleCall* speckle, const rtDecodeCall* decode, const rtVoxelCall* voxel, rtStream stream) {
    if (!voxel) return rt_net_execute_frames_camera(net, call, out, rect, speckle, decode, stream);
    FrameJob j;
    j.c = call;
    j.d = out;
    j.r = rect;
    j.sp = speckle;
    j.dec = decode;
    j.vx = voxel;
    return run_frames("rt_net_execute_frames_voxels: ", net, j, stream);
}

extern "C" int rt_net_profile(rtStereoNet* net, const void* left, const void* right, void* disp, int batch, char* buf,
                              size_t buf_bytes) {
    if (!net || !buf || !buf_bytes) return fail("rt_net_profile: null pointer");
    TextProfiler prof;
    net->context->setProfiler(&prof);
    void* bindings[3] = {const_cast<void*>(left), const_cast<void*>(right), disp};
    const bool ok = net->context->execute(batch, bindings);
    net->context->setProfiler(nullptr);
    if (!ok) return fail("rt_net_profile: " + net->log.last_error);
    std::ostringstream s;
    for (auto& r : prof.rows) s << r.first << "\t" << r.second << "\n";
    const std::string t = s.str();
    snprintf(buf, buf_bytes, "%s", t.c_str());
    return 0;
}

extern "C" int rt_net_set_streams(rtStereoNet* net, int streams) {
    if (!net || !net->context) return fail("rt_net_set_streams: null pointer");
    if (streams < 1 || streams > 2) return fail("rt_net_set_streams: 1 or 2 streams");
    net->context->setExecutionStreams(streams);
    return 0;
}

extern "C" int rt_net_set_graph(rtStereoNet* net, int on) {
    if (!net || !net->context) return fail("rt_net_set_graph: null pointer");
    net->context->setGraphMode(on != 0);
    return 0;
}

extern "C" int rt_net_set_launch_trace(rtStereoNet* net, int on) {
    if (!net || !net->context) return fail("rt_net_set_launch_trace: null pointer");
    net->context->setLaunchTrace(on != 0);
    return 0;
}

extern "C" int rt_net_read_launch_trace(rtStereoNet* net, unsigned long long* hashes, int max) {
    if (!net || !net->context || !hashes) { fail("rt_net_read_launch_trace: null pointer"); return -1; }
    const int n = net->context->readLaunchTrace(hashes, max);
    if (n < 0) fail("rt_net_read_launch_trace: read-back failed");
    return n;
}

extern "C" const char* rt_net_launch_name(const rtStereoNet* net, int launch) {
    return net && net->context ? net->context->getLaunchName(launch) : nullptr;
}

extern "C" long long rt_net_read_launch_output(rtStereoNet* net, int launch, void* host, long long bytes) {
    if (!net || !net->context) { fail("rt_net_read_launch_output: null pointer"); return -1; }
    const long long n = net->context->readLaunchOutput(launch, host, bytes);
    if (n < 0) fail("rt_net_read_launch_output: no traced pass, bad launch index or buffer too small");
    return n;
}

extern "C" int rt_net_num_layers(const rtStereoNet* net) { return net ? net->layers : 0; }
extern "C" int rt_net_num_launches(const rtStereoNet* net) { return net && net->engine ? net->engine->getNbLayers() : 0; }
extern "C" int rt_net_destroy(rtStereoNet* net) {
    delete net;
    return 0;
}
