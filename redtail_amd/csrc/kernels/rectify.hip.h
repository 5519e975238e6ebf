// Rectification of raw camera frames (what image_proc / stereo_image_proc do in front of a stereo node): the map of
// cv::initUndistortRectifyMap evaluated per pixel in double, and cv::remap(INTER_LINEAR, BORDER_CONSTANT, 0) in fp32 on the u8 frames.
// include/rt_stereo.h carries the full statement (rt_rectify_frames_u8); every operation here is rounded on its own.
#pragma once
#include "common.hip.h"
#include "imgproc.hip.h"

namespace rt {

struct RectifyCam {              // rtRectifyCamera, field for field
    double fx, fy, cx, cy;
    double d[8];                 // k1 k2 p1 p2 k3 k4 k5 k6
    double iR[9];
};

// the source position of destination pixel (row, col): pinhole ray through inv(P[:, :3] * R), plumb_bob / rational_polynomial distortion, K
__device__ static __forceinline__ void rectify_position(const RectifyCam& c, int col, int row, float& mx, float& my) {
#pragma clang fp contract(off)
    const double u = (double)col, v = (double)row;
    const double X = (c.iR[0] * u + c.iR[1] * v) + c.iR[2];
    const double Y = (c.iR[3] * u + c.iR[4] * v) + c.iR[5];
    const double W = (c.iR[6] * u + c.iR[7] * v) + c.iR[8];
    const double x = X / W, y = Y / W;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2.0 * x) * y;
    const double k1 = c.d[0], k2 = c.d[1], p1 = c.d[2], p2 = c.d[3], k3 = c.d[4], k4 = c.d[5], k5 = c.d[6], k6 = c.d[7];
    const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
    mx = (float)(c.fx * xd + c.cx);
    my = (float)(c.fy * yd + c.cy);
}

// rt_rectify_maps: the CV_32FC1 pair of one camera.  grid = (ceil(dw/64), ceil(dh/4))
__global__ void __launch_bounds__(256)
rectify_maps_kernel(RectifyCam cam, float* __restrict__ map_x, float* __restrict__ map_y, int dh, int dw) {
    const int dx = blockIdx.x * kFramesCols + threadIdx.x % kFramesCols, dy = blockIdx.y * kFramesRows + threadIdx.x / kFramesCols;
    if (dx >= dw || dy >= dh) return;
    float mx, my;
    rectify_position(cam, dx, dy, mx, my);
    const int64_t o = (int64_t)dy * dw + dx;
    map_x[o] = mx;
    map_y[o] = my;
}

struct RectifyArgs {
    const unsigned char *left, *right;   // source frames: sh x sw pixels, rows `step` bytes apart, frame n at n * sh * step
    int sh, sw;
    int64_t step;
    unsigned char *dleft, *dright;       // destination frames, the same encoding: dh x dw pixels, rows dstep bytes apart
    int dh, dw;
    int64_t dstep;
    int batch;
    const float *mxl, *myl, *mxr, *myr;  // MAP: (dh, dw) planes of the left and the right camera
    RectifyCam cam[2];                   // !MAP: left, right
};

// One pixel of the source as its bytes in memory order, byte c in bits 8c
template <int BPP, bool DWORD>
__device__ static __forceinline__ unsigned rectify_load(const unsigned char* px) {
    if constexpr (DWORD) {
        return *reinterpret_cast<const unsigned*>(px);
    } else {
        unsigned v = (unsigned)px[0] | ((unsigned)px[1] << 8) | ((unsigned)px[2] << 16);
        if constexpr (BPP == 4) v |= (unsigned)px[3] << 24;
        return v;
    }
}

// Both frames of a pair batch through the sampler, positions from the camera model (!MAP: formed in registers, no map is written) or
// from maps.  The house shape of the frame kernels: a block is 64 destination columns x 4 rows, one wave per row, so neighbouring lanes
// gather neighbouring source pixels and the caches serve the taps.  A pixel's four taps are loaded, all bytes of them, at clamped
// addresses before the first is used; a tap outside the image then counts as 0.  All channels (alpha included) take
//   top = S00 * (1 - a) + S01 * a,  bot = S10 * (1 - a) + S11 * a,  v = top * (1 - b) + bot * b,  byte = rintf(v)        (fp32, uncontracted)
// DWORD (4-byte pixels, every base and step a multiple of 4): one dword load per tap and one dword store per pixel, 256 contiguous bytes
// a wave.  3-byte pixels: the wave's 192 bytes are laid into LDS at the alignment they have in memory, and lane j stores the j-th aligned
// dword of that span; only a dword cut by the span's first or last byte -- the row's ends, and the seams between blocks of a row that
// starts off a dword -- is stored byte by byte.  Bytes behind a row's last pixel are never written.
// grid = (ceil(dw/64), ceil(dh/4), 2 * batch): z < batch -> left frame z, else right frame z - batch
constexpr int kRectifySpanDwords = (3 * kFramesCols + 3 + 3) / 4;
template <int BPP, bool DWORD, bool MAP>
__global__ void __launch_bounds__(256)
rectify_frames_kernel(RectifyArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned s_span[kFramesRows][kRectifySpanDwords + 1];
    const int tx = threadIdx.x % kFramesCols, ty = threadIdx.x / kFramesCols;
    const int dx = blockIdx.x * kFramesCols + tx, dy = blockIdx.y * kFramesRows + ty;
    const bool second = (int)blockIdx.z >= a.batch;
    const int n = second ? blockIdx.z - a.batch : blockIdx.z;
    if (dy >= a.dh) return;                            // a whole wave: ty is the wave index
    const unsigned char* s = (second ? a.right : a.left) + (int64_t)n * a.sh * a.step;
    unsigned char* drow = (second ? a.dright : a.dleft) + ((int64_t)n * a.dh + dy) * a.dstep;
    unsigned px = 0u;                                  // the destination pixel's bytes, byte c in bits 8c
    if (dx < a.dw) {
        float mx, my;
        if constexpr (MAP) {
            const int64_t o = (int64_t)dy * a.dw + dx;
            mx = (second ? a.mxr : a.mxl)[o];
            my = (second ? a.myr : a.myl)[o];
        } else {
            rectify_position(a.cam[second ? 1 : 0], dx, dy, mx, my);
        }
        if (mx > -1.f && mx < (float)a.sw && my > -1.f && my < (float)a.sh) {      // (false for a NaN; nothing was made an integer yet)
            const float fx0 = floorf(mx), fy0 = floorf(my);
            const float wa = mx - fx0, wb = my - fy0, ua = 1.f - wa, ub = 1.f - wb;
            const int x0 = (int)fx0, y0 = (int)fy0;                                  // in [-1, sw - 1] and [-1, sh - 1]
            const bool vx0 = x0 >= 0, vx1 = x0 + 1 < a.sw, vy0 = y0 >= 0, vy1 = y0 + 1 < a.sh;
            const unsigned char* r0 = s + (int64_t)(vy0 ? y0 : 0) * a.step;
            const unsigned char* r1 = s + (int64_t)(vy1 ? y0 + 1 : a.sh - 1) * a.step;
            const int o0 = (vx0 ? x0 : 0) * BPP, o1 = (vx1 ? x0 + 1 : a.sw - 1) * BPP;
            unsigned t00 = rectify_load<BPP, DWORD>(r0 + o0), t01 = rectify_load<BPP, DWORD>(r0 + o1);
            unsigned t10 = rectify_load<BPP, DWORD>(r1 + o0), t11 = rectify_load<BPP, DWORD>(r1 + o1);
            t00 = vx0 && vy0 ? t00 : 0u; t01 = vx1 && vy0 ? t01 : 0u;
            t10 = vx0 && vy1 ? t10 : 0u; t11 = vx1 && vy1 ? t11 : 0u;
#pragma unroll
            for (int c = 0; c < BPP; c++) {
                const float s00 = (float)((t00 >> (8 * c)) & 0xffu), s01 = (float)((t01 >> (8 * c)) & 0xffu);
                const float s10 = (float)((t10 >> (8 * c)) & 0xffu), s11 = (float)((t11 >> (8 * c)) & 0xffu);
                const float top = s00 * ua + s01 * wa;
                const float bot = s10 * ua + s11 * wa;
                const float v = top * ub + bot * wb;
                px |= (unsigned)rintf(v) << (8 * c);
            }
        }
    }
    if constexpr (BPP == 4) {
        if (dx >= a.dw) return;
        if constexpr (DWORD) {
            *reinterpret_cast<unsigned*>(drow + (int64_t)dx * 4) = px;
        } else {
            unsigned char* p = drow + (int64_t)dx * 4;
            p[0] = (unsigned char)px; p[1] = (unsigned char)(px >> 8); p[2] = (unsigned char)(px >> 16); p[3] = (unsigned char)(px >> 24);
        }
    } else {
        unsigned char* span = drow + (int64_t)blockIdx.x * (3 * kFramesCols);         // the wave's first byte
        const int al = (int)(reinterpret_cast<uintptr_t>(span) & 3);                  // it lies `al` bytes past a dword
        const int left = a.dw - (int)blockIdx.x * kFramesCols;
        const int bytes = 3 * (left < kFramesCols ? left : kFramesCols);
        unsigned char* lds = reinterpret_cast<unsigned char*>(s_span[ty]);
        if (dx < a.dw) {
            lds[al + 3 * tx] = (unsigned char)px; lds[al + 3 * tx + 1] = (unsigned char)(px >> 8); lds[al + 3 * tx + 2] = (unsigned char)(px >> 16);
        }
        wave_lds_sync();
        const int b0 = 4 * tx - al;                    // span byte at which this lane's dword starts (< 0: the span's head)
        if (b0 >= bytes) return;
        const unsigned v = s_span[ty][tx];
        if (b0 >= 0 && b0 + 4 <= bytes) {
            *reinterpret_cast<unsigned*>(span + b0) = v;
        } else {
            for (int j = 0; j < 4; j++)
                if (b0 + j >= 0 && b0 + j < bytes) span[b0 + j] = (unsigned char)(v >> (8 * j));
        }
    }
}

}  // namespace rt
