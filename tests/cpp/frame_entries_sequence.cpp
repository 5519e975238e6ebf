// The sequence of tests/test_frame_entries.py through the C ABI, as a stand-alone program: one ResNet-18 2D net (41 x 25, max_batch 4), all
// seven rt_net_execute_frames* entries at batch 1 and 2 in the same interleaved order, refused calls between them, then rt_net_destroy.
// It checks return codes only; what the calls write is tests/test_frame_entries.py's business.  Its purpose is a host-side sanitizer run
// of redtail_amd/csrc/host/ (the net's buffers on the normal and on the error paths) on the CPU, against the emulator build of the kernels:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I redtail_amd/include \
//       tests/cpp/frame_entries_sequence.cpp redtail_amd/csrc/host/{plugins,engine,networks,net_capi}.cpp \
//       -L tests/emu/build -l:librt_stereo_emu.so -Wl,-rpath,$PWD/tests/emu/build -o frame_entries_sequence
//   ./frame_entries_sequence weights.bin           (weights.bin: redtail_amd.capi.pack_weights(oracle.stereo_oracle.synth_weights_resnet18_2d()))
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_stereo.h"
#include "rt_stereo_net.h"

namespace {

constexpr int W = 41, H = 25, PAD = 13, ENC = RT_ENC_BGRA8;
int failures = 0;

struct Frames {                                    // a pair batch of 2 random bgra8 frames with padded rows, on the device
    int h, w;
    int64_t step;
    void *left = nullptr, *right = nullptr;
    Frames(int h_, int w_, unsigned seed) : h(h_), w(w_), step(4 * w_ + PAD) {
        std::vector<unsigned char> host(2 * (size_t)h * step);
        for (void** p : {&left, &right}) {
            for (auto& b : host) b = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
            if (rt_malloc(p, host.size()) != 0 || rt_memcpy_h2d(*p, host.data(), host.size(), nullptr) != 0) abort();
        }
        rt_stream_sync(nullptr);
    }
    ~Frames() {
        rt_free(left);
        rt_free(right);
    }
};

struct Outputs {                                   // every output an entry can write, large enough for batch 2 of the larger frame
    void *disp, *disp_right, *mask, *valid_count, *depth, *points, *compact, *count, *viz;
    Outputs() {
        const size_t plane = 2 * 51 * 83;
        for (void** p : {&disp, &disp_right, &depth}) rt_malloc(p, 4 * plane);
        for (void** p : {&points, &compact}) rt_malloc(p, 16 * plane);
        rt_malloc(&mask, plane);
        rt_malloc(&valid_count, 16);
        rt_malloc(&count, 16);
        rt_malloc(&viz, 2 * (size_t)(2 * H) * (6 * W + PAD));
    }
    ~Outputs() {
        for (void* p : {disp, disp_right, mask, valid_count, depth, points, compact, count, viz}) rt_free(p);
    }
};

void expect(const char* what, int rc, int want) {
    if (rc == want) return;
    failures++;
    fprintf(stderr, "%s: returned %d, expected %d: %s\n", what, rc, want, rt_net_last_error());
}

rtRectifyCamera rectify_camera(int h, int w, double shift) {
    const double K[9] = {40, 0, w / 2.0, 0, 40, h / 2.0, 0, 0, 1}, D[5] = {-0.17, 0.026, 1e-3, -5e-4, 0};
    const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, P[12] = {40, 0, w / 2.0 + shift, 0, 0, 40, h / 2.0, 0, 0, 0, 1, 0};
    rtRectifyCamera cam;
    if (rt_rectify_camera_from_info(K, D, 5, R, P, &cam) != 0) abort();
    return cam;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s weights.bin\n", argv[0]), 2;
    rtStereoNet* net = nullptr;
    if (rt_net_create(&net, RT_MODEL_RESNET18_2D, W, H, 4, RT_F32, 8, argv[1]) != 0) return fprintf(stderr, "%s\n", rt_net_last_error()), 2;
    {
        Frames small(30, 36, 1), large(51, 83, 2);
        Outputs o;
        const auto call = [&](const Frames& f, int n, int resize, int geometry, int kind, float max_diff, bool masked) {
            return rtFrameCall{sizeof(rtFrameCall), f.left, f.right, f.h, f.w, f.step, ENC, resize, o.disp, kind, geometry, max_diff,
                               masked ? o.mask : nullptr, masked ? o.valid_count : nullptr, n};
        };
        const auto cloud = [&](const Frames& f, bool organised) {
            return rtDepthCall{sizeof(rtDepthCall), rtStereoCamera{30.f, 31.f, f.w / 2 - 0.3f, f.h / 2 + 0.2f, 0.1f, 0.5f}, 0.05f, 40.f, o.depth,
                               RT_DEPTH_M_F32, organised ? o.points : nullptr, o.compact, o.count};
        };
        const auto rectify = [&](const Frames& f) {
            return rtRectifyCall{sizeof(rtRectifyCall), rectify_camera(f.h, f.w, 0.0), rectify_camera(f.h, f.w, -1.5), nullptr, nullptr, 0};
        };
        const rtSpeckleCall speckle = {sizeof(rtSpeckleCall), 6, 1.f};
        const int64_t vstep = 6 * W + PAD;
        rtFrameCall c;
        rtDepthCall d;
        rtRectifyCall r;

        c = call(small, 1, RT_RESIZE_CV_AREA, RT_GEOM_FRAME, RT_DISP_PIXELS_F32, 1.5f, true), d = cloud(small, false), r = rectify(small);
        expect("0 filtered", rt_net_execute_frames_filtered(net, &c, &d, &r, &speckle, nullptr), 0);
        expect("1 frames", rt_net_execute_frames(net, large.left, large.right, large.h, large.w, large.step, ENC, o.disp, RT_DISP_PIXELS_F32, 2, nullptr), 0);
        expect("2 lr", rt_net_execute_frames_lr(net, large.left, large.right, large.h, large.w, large.step, ENC, o.disp, RT_DISP_KITTI_U16, o.mask,
                                                o.disp_right, o.valid_count, 1.f, 1, nullptr), 0);
        c = call(large, 2, RT_RESIZE_AREA_DOWN, RT_GEOM_NET, RT_DISP_PIXELS_F32, -1.f, false);
        expect("3 ex", rt_net_execute_frames_ex(net, &c, nullptr), 0);
        c = call(large, 1, RT_RESIZE_AREA_DOWN, RT_GEOM_NET, RT_DISP_KITTI_U16, 1.f, true);
        expect("4 ex", rt_net_execute_frames_ex(net, &c, nullptr), 0);
        expect("5 frames, up-scaling", rt_net_execute_frames(net, small.left, small.right, small.h, small.w, small.step, ENC, o.disp, RT_DISP_PIXELS_F32, 2, nullptr),
               RT_E_BADARG);
        expect("6 viz", rt_net_execute_frames_viz(net, large.left, large.right, large.h, large.w, large.step, ENC, o.disp, o.viz, vstep, 24.f, -1.f, nullptr,
                                                  nullptr, 1, nullptr), 0);
        expect("7 viz", rt_net_execute_frames_viz(net, large.left, large.right, large.h, large.w, large.step, ENC, o.disp, o.viz, vstep, 24.f, 1.f, o.mask,
                                                  o.valid_count, 2, nullptr), 0);
        c = call(large, 2, RT_RESIZE_CV_AREA, RT_GEOM_FRAME, RT_DISP_PIXELS_F32, -1.f, false), d = cloud(large, true), r = rectify(large);
        expect("8 raw", rt_net_execute_frames_raw(net, &c, &d, &r, nullptr), 0);                  // rect and points_ws grow
        expect("9 filtered, no filter", rt_net_execute_frames_filtered(net, &c, &d, &r, nullptr, nullptr), 0);
        c = call(small, 1, RT_RESIZE_CV_AREA, RT_GEOM_NET, RT_DISP_PIXELS_F32, -1.f, false), d = cloud(small, false);
        expect("10 filtered, network geometry", rt_net_execute_frames_filtered(net, &c, &d, nullptr, &speckle, nullptr), RT_E_UNSUPPORTED);
        c = call(small, 2, RT_RESIZE_CV_AREA, RT_GEOM_FRAME, RT_DISP_KITTI_U16, 1.5f, true);
        expect("11 3d, no out", rt_net_execute_frames_3d(net, &c, nullptr, nullptr), 0);
        expect("12 ex", rt_net_execute_frames_ex(net, &c, nullptr), 0);
        c = call(small, 1, RT_RESIZE_CV_AREA, RT_GEOM_FRAME, RT_DISP_PIXELS_F32, -1.f, false);
        expect("13 filtered, no filter", rt_net_execute_frames_filtered(net, &c, &d, nullptr, nullptr, nullptr), 0);
        expect("14 3d", rt_net_execute_frames_3d(net, &c, &d, nullptr), 0);
        expect("15 lr, no tolerance", rt_net_execute_frames_lr(net, large.left, large.right, large.h, large.w, large.step, ENC, o.disp, RT_DISP_PIXELS_F32,
                                                               o.mask, nullptr, nullptr, -1.f, 1, nullptr), RT_E_BADARG);
        expect("raw, no rect", rt_net_execute_frames_raw(net, &c, &d, nullptr, nullptr), RT_E_BADARG);
        c.struct_bytes -= 8;
        expect("ex, wrong struct size", rt_net_execute_frames_ex(net, &c, nullptr), RT_E_BADARG);
        c = call(small, 3, RT_RESIZE_CV_AREA, RT_GEOM_FRAME, RT_DISP_PIXELS_F32, 1.5f, true), r = rectify(small);
        expect("raw, batch too large", rt_net_execute_frames_raw(net, &c, nullptr, &r, nullptr), RT_E_BADARG);
        c = call(small, 2, RT_RESIZE_CV_AREA, RT_GEOM_FRAME, RT_DISP_PIXELS_F32, 1.5f, true), d = cloud(small, false);
        expect("16 filtered", rt_net_execute_frames_filtered(net, &c, &d, &r, &speckle, nullptr), 0);
        expect("17 frames", rt_net_execute_frames(net, large.left, large.right, large.h, large.w, large.step, ENC, o.disp, RT_DISP_NET, 1, nullptr), 0);
    }
    expect("destroy", rt_net_destroy(net), 0);
    // a net that never ran a frame, and creators that fail
    expect("create + destroy", rt_net_create(&net, RT_MODEL_RESNET18_2D, W, H, 4, RT_F32, 8, argv[1]) || rt_net_destroy(net), 0);
    expect("create, no file", rt_net_create(&net, RT_MODEL_RESNET18_2D, W, H, 4, RT_F32, 8, "/nonexistent/weights.bin"), RT_E_BADARG);
    rtNetOptions opt = {};
    opt.model = RT_MODEL_RESNET18_2D, opt.width = W, opt.height = H, opt.max_batch = 1, opt.weights_dtype = RT_F32, opt.max_disp = 8;
    expect("create_opt, no weights", rt_net_create_opt(&net, &opt), RT_E_BADARG);
    opt.weights_path = argv[1];
    expect("create_opt + destroy", rt_net_create_opt(&net, &opt) || rt_net_destroy(net), 0);
    expect("create_broadcast, no image", rt_net_create_broadcast(&net, RT_MODEL_RESNET18_2D, W, H, 1, RT_F32, 8, nullptr, 0, nullptr, 0), RT_E_BADARG);
    printf("%s (%d unexpected return codes)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
