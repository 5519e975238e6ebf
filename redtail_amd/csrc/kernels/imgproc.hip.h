// Image front-end / back-end of the sample application on the GPU:
//   preprocess_bgr8_kernel   replaces readImgFile()'s cv::Mat pipeline (reference sample_app/main.cpp:83-98):
//                            u8 BGR HWC -> float, cv::resize(INTER_AREA), BGR -> RGB, HWC -> CHW, / 255
//   disparity_u16_kernel     replaces the result path (main.cpp:324-330): disparity * 256 (* width for the sigmoid
//                            output of ResNet-18 2D) -> saturating round-to-nearest-even conversion to 16 bit (KITTI PNG)
// so a camera frame crosses PCIe as 3 bytes per pixel instead of 12 and the host does no per-pixel work.
// INTER_AREA for down-scaling is the area-weighted box average of OpenCV's computeResizeAreaTab: destination pixel dx
// covers source interval [dx*s, (dx+1)*s), every source pixel contributes its overlap / cell width.
#pragma once
#include "common.hip.h"

namespace rt {

// overlap weights of destination index `d` along one axis (scale s >= 1, source size n): first source index and up
// to kMaxTaps weights, exactly as OpenCV builds its table (fractional head, whole pixels, fractional tail).
constexpr int kAreaMaxTaps = 8;       // supports scale factors up to 6
// (positions in double like OpenCV's table builder -- d * s in fp32 is off by 1e-4 pixels at x = 1000 -- weights float)
__device__ static __forceinline__ int area_taps(int d, double s, int n, float* wgt) {
    const double f1 = d * s, f2 = f1 + s;
    const double cell = fmin(s, (double)n - f1);
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = s2 < n ? s2 : n;
    s1 = s1 < s2 ? s1 : s2;
    int first = s1, k = 0;
    if (s1 - f1 > 1e-3) { first = s1 - 1; wgt[k++] = (float)((s1 - f1) / cell); }
    for (int sx = s1; sx < s2 && k < kAreaMaxTaps; sx++) wgt[k++] = (float)(1.0 / cell);
    if (f2 - s2 > 1e-3 && k < kAreaMaxTaps && s2 < n) wgt[k++] = (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell);
    for (int i = k; i < kAreaMaxTaps; i++) wgt[i] = 0.f;
    return first;
}

// grid = (ceil(dw/256), dh, batch)
__global__ void __launch_bounds__(256)
preprocess_bgr8_kernel(const unsigned char* __restrict__ src, int sh, int sw, float* __restrict__ dst, int dh, int dw) {
    const int dx = blockIdx.x * 256 + threadIdx.x, dy = blockIdx.y, n = blockIdx.z;
    if (dx >= dw) return;
    const unsigned char* s = src + (int64_t)n * sh * sw * 3;
    float* d = dst + (int64_t)n * 3 * dh * dw;
    float b = 0.f, g = 0.f, r = 0.f;
    if (sh == dh && sw == dw) {
        const unsigned char* px = s + ((int64_t)dy * sw + dx) * 3;
        b = px[0]; g = px[1]; r = px[2];
    } else {
        float wx[kAreaMaxTaps], wy[kAreaMaxTaps];
        const int x0 = area_taps(dx, (double)sw / dw, sw, wx);
        const int y0 = area_taps(dy, (double)sh / dh, sh, wy);
        for (int j = 0; j < kAreaMaxTaps; j++) {
            if (wy[j] == 0.f) continue;
            const unsigned char* row = s + (int64_t)(y0 + j) * sw * 3;
            float rb = 0.f, rg = 0.f, rr = 0.f;
            for (int i = 0; i < kAreaMaxTaps; i++) {
                if (wx[i] == 0.f) continue;
                const unsigned char* px = row + (x0 + i) * 3;
                rb += wx[i] * px[0]; rg += wx[i] * px[1]; rr += wx[i] * px[2];
            }
            b += wy[j] * rb; g += wy[j] * rg; r += wy[j] * rr;
        }
    }
    const int64_t plane = (int64_t)dh * dw, o = (int64_t)dy * dw + dx;
    d[o] = r / 255.f;                 // RGB planes
    d[plane + o] = g / 255.f;
    d[2 * plane + o] = b / 255.f;
}

// Both frames of a stereo pair as a camera driver delivers them (reference ros/packages/stereo_dnn_ros/src/stereo_dnn_ros_node.cpp:
// 42-58, 60-77): sensor_msgs/Image rows `step` bytes apart, 3 or 4 bytes per pixel in B,G,R(,A) or R,G,B(,A) order; alpha is dropped
// (cv::cvtColor CV_BGRA2RGB).  Same filter, tap order and per-channel accumulation order as preprocess_bgr8_kernel, so the result is
// bit-identical to it on the dense BGR form of the same pixels.  A block is 64 destination columns x 4 rows: the x taps of its 64
// columns and the y taps of its 4 rows are built once into LDS (by wave 0 and by lanes 0-3 of wave 1) instead of in every thread.
// Each wave stores 64 consecutive floats of one row per plane.
// grid = (ceil(dw/64), ceil(dh/4), 2 * batch): z < batch -> left frame z, else right frame z - batch
constexpr int kFramesCols = 64, kFramesRows = 4;
template <int BPP, bool DWORD>          // DWORD: 4-byte pixels at 4-byte aligned addresses, one dword load per tap
__global__ void __launch_bounds__(256)
preprocess_frames_kernel(const unsigned char* __restrict__ left, const unsigned char* __restrict__ right, int sh, int sw, int64_t step,
                         bool rgb_order, float* __restrict__ dleft, float* __restrict__ dright, int dh, int dw, int batch) {
    __shared__ float s_wx[kAreaMaxTaps][kFramesCols];
    __shared__ float s_wy[kFramesRows][kAreaMaxTaps];
    __shared__ int s_x0[kFramesCols], s_y0[kFramesRows];
    const int tx = threadIdx.x % kFramesCols, ty = threadIdx.x / kFramesCols;
    const int dx = blockIdx.x * kFramesCols + tx, dy = blockIdx.y * kFramesRows + ty;
    const bool second = (int)blockIdx.z >= batch;
    const int n = second ? blockIdx.z - batch : blockIdx.z;
    const unsigned char* s = (second ? right : left) + (int64_t)n * sh * step;
    float* d = (second ? dright : dleft) + (int64_t)n * 3 * dh * dw;
    const bool resize = !(sh == dh && sw == dw);
    if (resize) {                                      // (uniform over the grid: every thread reaches the barrier or none does)
        if (ty == 0 && dx < dw) {
            float wx[kAreaMaxTaps];
            s_x0[tx] = area_taps(dx, (double)sw / dw, sw, wx);
            for (int i = 0; i < kAreaMaxTaps; i++) s_wx[i][tx] = wx[i];
        } else if (ty == 1 && tx < kFramesRows && (int)blockIdx.y * kFramesRows + tx < dh) {
            s_y0[tx] = area_taps(blockIdx.y * kFramesRows + tx, (double)sh / dh, sh, s_wy[tx]);
        }
        __syncthreads();
    }
    if (dx >= dw || dy >= dh) return;
    auto pixel = [&](const unsigned char* px, unsigned& c0, unsigned& c1, unsigned& c2) {
        if constexpr (DWORD) {
            const unsigned v = *reinterpret_cast<const unsigned*>(px);
            c0 = v & 0xffu; c1 = (v >> 8) & 0xffu; c2 = (v >> 16) & 0xffu;
        } else {
            c0 = px[0]; c1 = px[1]; c2 = px[2];
        }
    };
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;               // channels in memory order: B,G,R or R,G,B
    if (!resize) {
        unsigned c0, c1, c2;
        pixel(s + (int64_t)dy * step + (int64_t)dx * BPP, c0, c1, c2);
        a0 = c0; a1 = c1; a2 = c2;
    } else {
        float wx[kAreaMaxTaps], wy[kAreaMaxTaps];
        for (int i = 0; i < kAreaMaxTaps; i++) { wx[i] = s_wx[i][tx]; wy[i] = s_wy[ty][i]; }
        const int x0 = s_x0[tx], y0 = s_y0[ty];
        for (int j = 0; j < kAreaMaxTaps; j++) {
            if (wy[j] == 0.f) continue;
            const unsigned char* row = s + (int64_t)(y0 + j) * step;
            float r0 = 0.f, r1 = 0.f, r2 = 0.f;
            for (int i = 0; i < kAreaMaxTaps; i++) {
                if (wx[i] == 0.f) continue;
                unsigned c0, c1, c2;
                pixel(row + (x0 + i) * BPP, c0, c1, c2);
                r0 += wx[i] * c0; r1 += wx[i] * c1; r2 += wx[i] * c2;
            }
            a0 += wy[j] * r0; a1 += wy[j] * r1; a2 += wy[j] * r2;
        }
    }
    const float r = rgb_order ? a0 : a2, g = a1, b = rgb_order ? a2 : a0;
    const int64_t plane = (int64_t)dh * dw, o = (int64_t)dy * dw + dx;
    d[o] = r / 255.f;                 // RGB planes
    d[plane + o] = g / 255.f;
    d[2 * plane + o] = b / 255.f;
}

// The pair batch of preprocess_frames_kernel plus its mirrored, swapped twin for the left-right consistency check: dleft / dright hold
// 2 * batch images, images [0, batch) are what preprocess_frames_kernel writes (same taps, same accumulation order: bit-identical) and
//   dleft[batch + n](c, y, x) = dright[n](c, y, dw-1-x),   dright[batch + n](c, y, x) = dleft[n](c, y, dw-1-x)
// so that the engine's output for image batch + n, mirrored, is the disparity of the right view.  Every value is computed once and stored
// twice; the u8 frames are read once.  The mirrored copy of a wave's 64 columns [c0, c0+63] is the span [dw-64-c0, dw-1-c0], again 256
// contiguous bytes.  The values are reversed across the wave in registers (lane l takes lane 63-l's), so lane l stores column
// dw-64-c0+l: consecutive lanes write consecutive addresses, exactly as in the forward store, instead of walking the span backwards.
// Lanes past the row's end stay in the wave until the exchange is done (they hold nothing and store nothing).
// grid = (ceil(dw/64), ceil(dh/4), 2 * batch): z < batch -> left frame z, else right frame z - batch
template <int BPP, bool DWORD>
__global__ void __launch_bounds__(256)
preprocess_frames_lr_kernel(const unsigned char* __restrict__ left, const unsigned char* __restrict__ right, int sh, int sw, int64_t step,
                            bool rgb_order, float* __restrict__ dleft, float* __restrict__ dright, int dh, int dw, int batch) {
    __shared__ float s_wx[kAreaMaxTaps][kFramesCols];
    __shared__ float s_wy[kFramesRows][kAreaMaxTaps];
    __shared__ int s_x0[kFramesCols], s_y0[kFramesRows];
    const int tx = threadIdx.x % kFramesCols, ty = threadIdx.x / kFramesCols;
    const int dx = blockIdx.x * kFramesCols + tx, dy = blockIdx.y * kFramesRows + ty;
    const bool second = (int)blockIdx.z >= batch;
    const int n = second ? blockIdx.z - batch : blockIdx.z;
    const unsigned char* s = (second ? right : left) + (int64_t)n * sh * step;
    const int64_t plane = (int64_t)dh * dw;
    float* d = (second ? dright : dleft) + (int64_t)n * 3 * plane;
    float* m = (second ? dleft : dright) + (int64_t)(batch + n) * 3 * plane;       // the mirrored copy goes to the other side
    const bool resize = !(sh == dh && sw == dw);
    if (resize) {                                      // (uniform over the grid: every thread reaches the barrier or none does)
        if (ty == 0 && dx < dw) {
            float wx[kAreaMaxTaps];
            s_x0[tx] = area_taps(dx, (double)sw / dw, sw, wx);
            for (int i = 0; i < kAreaMaxTaps; i++) s_wx[i][tx] = wx[i];
        } else if (ty == 1 && tx < kFramesRows && (int)blockIdx.y * kFramesRows + tx < dh) {
            s_y0[tx] = area_taps(blockIdx.y * kFramesRows + tx, (double)sh / dh, sh, s_wy[tx]);
        }
        __syncthreads();
    }
    if (dy >= dh) return;                              // a whole wave: ty is the wave index
    auto pixel = [&](const unsigned char* px, unsigned& c0, unsigned& c1, unsigned& c2) {
        if constexpr (DWORD) {
            const unsigned v = *reinterpret_cast<const unsigned*>(px);
            c0 = v & 0xffu; c1 = (v >> 8) & 0xffu; c2 = (v >> 16) & 0xffu;
        } else {
            c0 = px[0]; c1 = px[1]; c2 = px[2];
        }
    };
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;               // channels in memory order: B,G,R or R,G,B
    if (dx < dw) {
        if (!resize) {
            unsigned c0, c1, c2;
            pixel(s + (int64_t)dy * step + (int64_t)dx * BPP, c0, c1, c2);
            a0 = c0; a1 = c1; a2 = c2;
        } else {
            float wx[kAreaMaxTaps], wy[kAreaMaxTaps];
            for (int i = 0; i < kAreaMaxTaps; i++) { wx[i] = s_wx[i][tx]; wy[i] = s_wy[ty][i]; }
            const int x0 = s_x0[tx], y0 = s_y0[ty];
            for (int j = 0; j < kAreaMaxTaps; j++) {
                if (wy[j] == 0.f) continue;
                const unsigned char* row = s + (int64_t)(y0 + j) * step;
                float r0 = 0.f, r1 = 0.f, r2 = 0.f;
                for (int i = 0; i < kAreaMaxTaps; i++) {
                    if (wx[i] == 0.f) continue;
                    unsigned c0, c1, c2;
                    pixel(row + (x0 + i) * BPP, c0, c1, c2);
                    r0 += wx[i] * c0; r1 += wx[i] * c1; r2 += wx[i] * c2;
                }
                a0 += wy[j] * r0; a1 += wy[j] * r1; a2 += wy[j] * r2;
            }
        }
    }
    const float r = (rgb_order ? a0 : a2) / 255.f, g = a1 / 255.f, b = (rgb_order ? a2 : a0) / 255.f;
    const int64_t o = (int64_t)dy * dw + dx;
    if (dx < dw) {
        d[o] = r;                     // RGB planes
        d[plane + o] = g;
        d[2 * plane + o] = b;
    }
    const float mr = __shfl(r, kFramesCols - 1 - tx), mg = __shfl(g, kFramesCols - 1 - tx), mb = __shfl(b, kFramesCols - 1 - tx);
    const int mx = dw - kFramesCols - (int)blockIdx.x * kFramesCols + tx;      // = dw-1 - (column of lane 63-tx); < 0: that lane is past the row
    if (mx >= 0) {
        const int64_t mo = (int64_t)dy * dw + mx;
        m[mo] = mr;
        m[plane + mo] = mg;
        m[2 * plane + mo] = mb;
    }
}

// cv::resize(INTER_AREA) when either axis grows (reference stereo_dnn_ros_node.cpp:42-58 calls it for whatever the camera sends).
// OpenCV has true area interpolation for shrinking both ways only; otherwise BOTH axes -- the shrinking one included -- take the two-tap
// set-up of its area_mode branch.  Per axis, source size n, destination size m, destination index d, positions in double, weight fp32:
//   inv = (double)m / n,  scale = 1.0 / inv,  s = (int)floor(d * scale),  f = (float)((d + 1) - (s + 1) * inv),
//   f = f <= 0 ? 0 : f - floorf(f),  s >= n - 1: s = n - 1, f = 0;   taps: s with weight 1.f - f, min(s + 1, n - 1) with weight f
// (s + 1) * inv is rounded before the subtraction (no FMA): where d * scale lands on an integer the weight depends on it.
__device__ static __forceinline__ void cv_area_tap(int d, int n, int m, int& s0, int& s1, float& w1) {
#pragma clang fp contract(off)
    const double inv = (double)m / (double)n, scale = 1.0 / inv;
    int s = (int)floor((double)d * scale);
    const double t = (double)(s + 1) * inv;
    float f = (float)((double)(d + 1) - t);
    f = f <= 0.f ? 0.f : f - floorf(f);
    if (s >= n - 1) { s = n - 1; f = 0.f; }
    s0 = s;
    s1 = s + 1 < n ? s + 1 : n - 1;
    w1 = f;
}

template <int BPP, bool DWORD>
__device__ static __forceinline__ void frame_pixel(const unsigned char* px, unsigned& c0, unsigned& c1, unsigned& c2) {
    if constexpr (DWORD) {
        const unsigned v = *reinterpret_cast<const unsigned*>(px);
        c0 = v & 0xffu; c1 = (v >> 8) & 0xffu; c2 = (v >> 16) & 0xffu;
    } else {
        c0 = px[0]; c1 = px[1]; c2 = px[2];
    }
}

// The pair batch of preprocess_frames_kernel (TWIN: plus the mirrored, swapped twin of preprocess_frames_lr_kernel, same exchange across
// the wave) through the two-tap filter above.  Same block shape: 64 destination columns x 4 rows, the x taps of the columns and the y taps
// of the rows built once into LDS (double-precision work) by wave 0 and by lanes 0-3 of wave 1.  A pixel has four source pixels, all
// loaded before the first is used.  Per channel, fp32, x first, every product and sum rounded on its own (contraction is off):
//   row_j = S[y_j][x0] * a0 + S[y_j][x1] * a1,   v = row_0 * b0 + row_1 * b1,   then colour order, / 255, planes as preprocess_frames_kernel
// grid = (ceil(dw/64), ceil(dh/4), 2 * batch): z < batch -> left frame z, else right frame z - batch
template <int BPP, bool DWORD, bool TWIN>
__global__ void __launch_bounds__(256)
preprocess_frames_cv_kernel(const unsigned char* __restrict__ left, const unsigned char* __restrict__ right, int sh, int sw, int64_t step,
                            bool rgb_order, float* __restrict__ dleft, float* __restrict__ dright, int dh, int dw, int batch) {
#pragma clang fp contract(off)
    __shared__ int s_x0[kFramesCols], s_x1[kFramesCols], s_y0[kFramesRows], s_y1[kFramesRows];
    __shared__ float s_a1[kFramesCols], s_b1[kFramesRows];
    const int tx = threadIdx.x % kFramesCols, ty = threadIdx.x / kFramesCols;
    const int dx = blockIdx.x * kFramesCols + tx, dy = blockIdx.y * kFramesRows + ty;
    const bool second = (int)blockIdx.z >= batch;
    const int n = second ? blockIdx.z - batch : blockIdx.z;
    const unsigned char* s = (second ? right : left) + (int64_t)n * sh * step;
    const int64_t plane = (int64_t)dh * dw;
    float* d = (second ? dright : dleft) + (int64_t)n * 3 * plane;
    if (ty == 0 && dx < dw) {
        cv_area_tap(dx, sw, dw, s_x0[tx], s_x1[tx], s_a1[tx]);
    } else if (ty == 1 && tx < kFramesRows && (int)blockIdx.y * kFramesRows + tx < dh) {
        cv_area_tap(blockIdx.y * kFramesRows + tx, sh, dh, s_y0[tx], s_y1[tx], s_b1[tx]);
    }
    __syncthreads();
    if (dy >= dh) return;                              // a whole wave: ty is the wave index
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;               // channels in memory order: B,G,R or R,G,B
    if (dx < dw) {
        const float a1 = s_a1[tx], a0 = 1.f - a1, b1 = s_b1[ty], b0 = 1.f - b1;
        const unsigned char* r0 = s + (int64_t)s_y0[ty] * step;
        const unsigned char* r1 = s + (int64_t)s_y1[ty] * step;
        const int64_t o0 = (int64_t)s_x0[tx] * BPP, o1 = (int64_t)s_x1[tx] * BPP;
        unsigned p[4][3];
        frame_pixel<BPP, DWORD>(r0 + o0, p[0][0], p[0][1], p[0][2]);
        frame_pixel<BPP, DWORD>(r0 + o1, p[1][0], p[1][1], p[1][2]);
        frame_pixel<BPP, DWORD>(r1 + o0, p[2][0], p[2][1], p[2][2]);
        frame_pixel<BPP, DWORD>(r1 + o1, p[3][0], p[3][1], p[3][2]);
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float top = (float)p[0][c] * a0 + (float)p[1][c] * a1;
            const float bot = (float)p[2][c] * a0 + (float)p[3][c] * a1;
            v[c] = top * b0 + bot * b1;
        }
        v0 = v[0]; v1 = v[1]; v2 = v[2];
    }
    const float r = (rgb_order ? v0 : v2) / 255.f, g = v1 / 255.f, b = (rgb_order ? v2 : v0) / 255.f;
    const int64_t o = (int64_t)dy * dw + dx;
    if (dx < dw) {
        d[o] = r;                     // RGB planes
        d[plane + o] = g;
        d[2 * plane + o] = b;
    }
    if constexpr (TWIN) {              // as preprocess_frames_lr_kernel: lanes past the row's end stay in the wave for the exchange
        float* m = (second ? dleft : dright) + (int64_t)(batch + n) * 3 * plane;
        const float mr = __shfl(r, kFramesCols - 1 - tx), mg = __shfl(g, kFramesCols - 1 - tx), mb = __shfl(b, kFramesCols - 1 - tx);
        const int mx = dw - kFramesCols - (int)blockIdx.x * kFramesCols + tx;
        if (mx >= 0) {
            const int64_t mo = (int64_t)dy * dw + mx;
            m[mo] = mr;
            m[plane + mo] = mg;
            m[2 * plane + mo] = mb;
        }
    }
}

// Left-right consistency check, mask and output encoding of a (2 * batch, 1, H, W) engine output whose images [batch, 2 batch) are the
// mirrored right views (preprocess_frames_lr_kernel).  All in fp32, every operation rounded on its own (contraction is off in this body):
//   dL(x) = L[y][x] * scale,  dR(x) = R[y][W-1-x] * scale,  xr = rintf((float)x - dL(x)),
//   valid = 0 <= xr <= W-1 and |dL(x) - dR(xr)| <= max_diff          (a NaN anywhere fails a comparison: not valid)
// A lane owns 4 consecutive pixels of one image's H*W plane, addressed as a flat run: rows of odd width make every row start at another
// alignment, a flat run of the plane has one alignment only.  Groups are laid so that their global element index is a multiple of 4
// (`vec`: all base pointers are 16-byte aligned): an image whose plane starts `a` elements past such a boundary gets a head group of
// 4 - a and a tail group of what is left, both done element by element by the lanes that own them; every other group is one 16-byte load
// of L, one 16-byte (fp32) / 8-byte (u16) store per output and one 4-byte mask store.  A group may cross from one row into the next: row
// and column are carried per element.  The right view's own pixels (right_out only) are one 16-byte load when the group lies in one row;
// the gather dR(xr) stays inside the row, at most the disparity range away from the lane's own columns: it is served by the caches.
// valid_count (zeroed by the host entry): a ballot per element slot, then one atomic per wave from its first lane.
// KIND: 0 raw network value, 1 pixels, 2 KITTI 16-bit (rintf(net * scale16) saturated; a valid 0 is raised to 1, an invalid pixel is 0)
// grid = (ceil(G / 256), batch) with G = (H*W + 6) / 4 groups: room for the head group
template <int KIND> struct LrOut { using type = float; };
template <> struct LrOut<2> { using type = unsigned short; };

template <int KIND>
__device__ static __forceinline__ typename LrOut<KIND>::type lr_encode(float net, float px, float scale16) {
    if constexpr (KIND == 0) return net;
    else if constexpr (KIND == 1) return px;
    else {
        const float v = rintf(net * scale16);         // as disparity_u16_kernel
        return (unsigned short)(v < 0.f ? 0.f : (v > 65535.f ? 65535.f : v));
    }
}

template <int KIND>
__global__ void __launch_bounds__(256)
lr_consistency_kernel(const float* __restrict__ net, int batch, int H, int W, float scale, float scale16, float max_diff,
                      void* __restrict__ out_v, unsigned char* __restrict__ mask, void* __restrict__ rout_v,
                      unsigned long long* __restrict__ count, int vec) {
#pragma clang fp contract(off)
    using T = typename LrOut<KIND>::type;
    const int n = blockIdx.y;
    const int64_t plane = (int64_t)H * W;
    const int64_t lbase = (int64_t)n * plane;
    const float* L = net + lbase;
    const float* R = net + (int64_t)(batch + n) * plane;
    T* out = static_cast<T*>(out_v) + lbase;
    T* rout = rout_v ? static_cast<T*>(rout_v) + lbase : nullptr;
    if (mask) mask += lbase;
    const int a = vec ? (int)(lbase & 3) : 0;
    const int64_t e0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x) - a;      // first element of the group, image-local (< 0 in the head group)
    const int lo = e0 < 0 ? (int)-e0 : 0;
    const int hi = e0 + 4 <= plane ? 4 : (int)(plane - e0);                    // <= 0: no element (lanes past the plane still vote below)
    const bool full = vec && lo == 0 && hi == 4;
    int y = 0, x = 0;
    if (lo < hi) {
        y = (int)((e0 + lo) / W);
        x = (int)((e0 + lo) - (int64_t)y * W);
    }
    float lv[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f};
    if (full) {
        const float4 v = *reinterpret_cast<const float4*>(L + e0);
        lv[0] = v.x; lv[1] = v.y; lv[2] = v.z; lv[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k >= lo && k < hi) lv[k] = L[e0 + k];
    }
    const bool one_row = full && x + 3 < W;
    if (rout && one_row) {                             // the right view's pixels x .. x+3 lie mirrored at W-4-x .. W-1-x (4-byte aligned only)
        float4 v;
        __builtin_memcpy(&v, R + (int64_t)y * W + (W - 4 - x), sizeof(v));
        rv[0] = v.w; rv[1] = v.z; rv[2] = v.y; rv[3] = v.x;
    }
    T ov[4], rov[4];
    unsigned ok[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool in = k >= lo && k < hi;
        const float dl = lv[k] * scale;
        const float xr = rintf((float)x - dl);
        bool valid = false;
        if (in && xr >= 0.f && xr <= (float)(W - 1)) {
            const float dr = R[(int64_t)y * W + (W - 1 - (int)xr)] * scale;
            valid = fabsf(dl - dr) <= max_diff;
        }
        if (rout && in && !one_row) rv[k] = R[(int64_t)y * W + (W - 1 - x)];
        T o = lr_encode<KIND>(lv[k], dl, scale16);
        if constexpr (KIND == 2) o = o == 0 ? (T)1 : o;
        ov[k] = valid ? o : (T)0;
        rov[k] = lr_encode<KIND>(rv[k], rv[k] * scale, scale16);
        ok[k] = valid ? 1u : 0u;
        if (in && ++x == W) { x = 0; y++; }
    }
    if (full) {
        if constexpr (KIND == 2) {
            *reinterpret_cast<uint2*>(out + e0) = make_uint2((unsigned)ov[0] | ((unsigned)ov[1] << 16), (unsigned)ov[2] | ((unsigned)ov[3] << 16));
            if (rout) *reinterpret_cast<uint2*>(rout + e0) = make_uint2((unsigned)rov[0] | ((unsigned)rov[1] << 16), (unsigned)rov[2] | ((unsigned)rov[3] << 16));
        } else {
            *reinterpret_cast<float4*>(out + e0) = make_float4(ov[0], ov[1], ov[2], ov[3]);
            if (rout) *reinterpret_cast<float4*>(rout + e0) = make_float4(rov[0], rov[1], rov[2], rov[3]);
        }
        if (mask) *reinterpret_cast<unsigned*>(mask + e0) = (ok[0] | (ok[1] << 8) | (ok[2] << 16) | (ok[3] << 24)) * 255u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < lo || k >= hi) continue;
            out[e0 + k] = ov[k];
            if (rout) rout[e0 + k] = rov[k];
            if (mask) mask[e0 + k] = (unsigned char)(ok[k] * 255u);
        }
    }
    if (count) {                                       // (uniform: every lane of every wave is still here)
        int c = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) c += __builtin_popcountll(__ballot(ok[k]));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(count + n, (unsigned long long)c);
    }
}

// Disparity of the network's geometry (H x W, pixels) -> the frame's geometry (oh x ow, the frame's pixels): bilinear with half-pixel
// centres (interpolate(mode="bilinear", align_corners=False)) times r = (float)ow / (float)W.  All fp32, contraction off.  Per axis
// (n source, m destination, index d):
//   sc = (float)n / (float)m,  p = max(((float)d + 0.5f) * sc - 0.5f, 0),  i0 = min((int)floorf(p), n - 1),  i1 = min(i0 + 1, n - 1),
//   w1 = p - (float)i0,  w0 = 1.f - w1
//   v = ((D[y0][x0] * a0 + D[y0][x1] * a1) * b0 + (D[y1][x0] * a0 + D[y1][x1] * a1) * b1) * r
// MASKED (the 255 / 0 mask of lr_consistency_kernel, network geometry): the nearest tap is x1 if a1 > 0.5f else x0, same in y; with all
// four taps valid v as above, otherwise v = D[nearest] * r (nothing is mixed with the zeros the check wrote); the frame pixel is valid iff
// its nearest tap is, an invalid one is 0 in out and in the mask; a valid 16-bit value that encodes to 0 is raised to 1.
// U16: rintf(v * 256.f) saturated to [0, 65535], NaN -> 0.
// Output addressing as lr_consistency_kernel: a lane owns 4 consecutive pixels of one image's oh * ow plane as a flat run, groups laid on
// 16-byte boundaries of the fp32 output (`vec`), head and tail groups element by element; row and column are carried per element.  The
// 16 gathers of a lane stay within two source rows per output row and are all issued before the first use.
// count (zeroed by the host entry): a ballot per element slot, the four waves' sums through LDS, one atomic per block -- one per wave,
// 1800 adds to one address for a 1242 x 375 frame, took the launch from 5.6 to 27.5 us.
// grid = (ceil(G / 256), batch) with G = (oh*ow + 6) / 4 groups
__device__ static __forceinline__ void frame_tap(int d, float sc, int n, int& i0, int& i1, float& w1) {
#pragma clang fp contract(off)
    float p = ((float)d + 0.5f) * sc - 0.5f;
    p = p < 0.f ? 0.f : p;
    const int i = (int)floorf(p);
    i0 = i < n - 1 ? i : n - 1;
    i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
    w1 = p - (float)i0;
}

template <bool U16, bool MASKED>
__global__ void __launch_bounds__(256)
disparity_to_frame_kernel(const float* __restrict__ disp, const unsigned char* __restrict__ mask, int H, int W, void* __restrict__ out_v,
                          int oh, int ow, unsigned char* __restrict__ omask, unsigned long long* __restrict__ count, int vec) {
#pragma clang fp contract(off)
    using T = typename LrOut<U16 ? 2 : 1>::type;
    const int n = blockIdx.y;
    const int64_t plane = (int64_t)oh * ow;
    const int64_t obase = (int64_t)n * plane;
    const float* D = disp + (int64_t)n * H * W;
    const unsigned char* M = MASKED ? mask + (int64_t)n * H * W : nullptr;
    T* out = static_cast<T*>(out_v) + obase;
    if (omask) omask += obase;
    const float sx = (float)W / (float)ow, sy = (float)H / (float)oh, r = (float)ow / (float)W;
    const int a = vec ? (int)(obase & 3) : 0;
    const int64_t e0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x) - a;      // first element of the group, image-local (< 0 in the head group)
    const int lo = e0 < 0 ? (int)-e0 : 0;
    const int hi = e0 + 4 <= plane ? 4 : (int)(plane - e0);                    // <= 0: no element (lanes past the plane still vote below)
    const bool full = vec && lo == 0 && hi == 4;
    int y = 0, x = 0;
    if (lo < hi) {
        y = (int)((e0 + lo) / ow);
        x = (int)((e0 + lo) - (int64_t)y * ow);
    }
    float t[4][4], a1[4], b1[4];
    unsigned m[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {                      // taps and loads of all four pixels first (clamped to pixel 0 for a slot without one)
        const bool in = k >= lo && k < hi;
        int x0, x1, y0, y1;
        frame_tap(in ? x : 0, sx, W, x0, x1, a1[k]);
        frame_tap(in ? y : 0, sy, H, y0, y1, b1[k]);
        const int64_t r0 = (int64_t)y0 * W, r1 = (int64_t)y1 * W;
        t[k][0] = D[r0 + x0]; t[k][1] = D[r0 + x1]; t[k][2] = D[r1 + x0]; t[k][3] = D[r1 + x1];
        if constexpr (MASKED) {
            m[k][0] = M[r0 + x0]; m[k][1] = M[r0 + x1]; m[k][2] = M[r1 + x0]; m[k][3] = M[r1 + x1];
        }
        if (in && ++x == ow) { x = 0; y++; }
    }
    T ov[4];
    unsigned ok[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool in = k >= lo && k < hi;
        const float a0 = 1.f - a1[k], b0 = 1.f - b1[k];
        const float top = t[k][0] * a0 + t[k][1] * a1[k];
        const float bot = t[k][2] * a0 + t[k][3] * a1[k];
        float v = (top * b0 + bot * b1[k]) * r;
        bool valid = in;
        if constexpr (MASKED) {
            const int nt = (b1[k] > 0.5f ? 2 : 0) + (a1[k] > 0.5f ? 1 : 0);
            const unsigned mn = nt == 0 ? m[k][0] : (nt == 1 ? m[k][1] : (nt == 2 ? m[k][2] : m[k][3]));
            const float tn = nt == 0 ? t[k][0] : (nt == 1 ? t[k][1] : (nt == 2 ? t[k][2] : t[k][3]));
            if (!(m[k][0] && m[k][1] && m[k][2] && m[k][3])) v = tn * r;
            valid = in && mn != 0;
        }
        T o;
        if constexpr (U16) {
            const float q = rintf(v * 256.f);
            o = (T)(q > 0.f ? (q < 65535.f ? q : 65535.f) : 0.f);              // NaN -> 0
            if (MASKED && o == 0) o = (T)1;
        } else {
            o = v;
        }
        ov[k] = valid ? o : (T)0;
        ok[k] = valid ? 1u : 0u;
    }
    if (full) {
        if constexpr (U16) *reinterpret_cast<uint2*>(out + e0) = make_uint2((unsigned)ov[0] | ((unsigned)ov[1] << 16), (unsigned)ov[2] | ((unsigned)ov[3] << 16));
        else *reinterpret_cast<float4*>(out + e0) = make_float4(ov[0], ov[1], ov[2], ov[3]);
        if (MASKED && omask) *reinterpret_cast<unsigned*>(omask + e0) = (ok[0] | (ok[1] << 8) | (ok[2] << 16) | (ok[3] << 24)) * 255u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < lo || k >= hi) continue;
            out[e0 + k] = ov[k];
            if (MASKED && omask) omask[e0 + k] = (unsigned char)(ok[k] * 255u);
        }
    }
    if (MASKED && count) {                             // (uniform: every lane of every wave is still here)
        __shared__ int s_count[4];
        int c = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) c += __builtin_popcountll(__ballot(ok[k]));
        if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            c = s_count[0] + s_count[1] + s_count[2] + s_count[3];
            if (c) atomicAdd(count + n, (unsigned long long)c);
        }
    }
}

// disparity_to_frame_kernel's resampling followed, in registers, by the reprojection of a rectified pair (stereo_image_proc's depth image
// and point cloud): per frame pixel (row y, column x), all fp32, contraction off, IEEE divisions:
//   v, valid0 = what disparity_to_frame_kernel forms      den = v + doffs      ok = valid0 && den > 0 && den finite
//   Z = fB / den  (fB = fx * baseline, formed on the host)   ok = ok && zmin <= Z <= zmax
//   X = (((float)x - cx) / fx) * Z      Y = (((float)y - cy) / fy) * Z
// Outputs, each optional (uniform branches on kernel arguments): the frame-geometry disparity, mask and count exactly as
// disparity_to_frame_kernel writes them; depth (fp32 metres, NaN = no value; or uint16 millimetres, 0 = no value, a valid 0 raised to 1);
// the organised cloud, one 16-byte record {X, Y, Z, R << 16 | G << 8 | B} per pixel (NaN coordinates where not ok, the colour always).
// Same lane-owns-4-pixels addressing as disparity_to_frame_kernel, the 16 gathers and the 4 colour pixels issued before their first use.
// Cloud records go through LDS so that one store instruction of the block covers 256 consecutive records (4 KB) instead of one record
// every 64 bytes: thread t leaves its records at slots 4t .. 4t + 3 and stores slots t, 256 + t, 512 + t, 768 + t.
// Compaction (valid points only, row-major, deterministic) without atomics and without one workgroup waiting for another:
//   !COMPACT: a block -- a "tile" of 1024 consecutive pixels -- leaves its number of ok pixels in tile_counts[n * tiles + blockIdx.x];
//   COMPACT (a second launch of the same grid, same `vec`): a block sums the counts of the tiles before it (strided loads, shuffles within
//   the wave, LDS across the four waves), forms its pixels again, and places them by ballot / popcount within the wave and the waves'
//   totals through LDS; the block of the last tile writes count[n].
// grid = (ceil(G / 256), batch) with G = (oh*ow + 6) / 4 groups
struct PointsArgs {
    const float* disp; const unsigned char* mask; int H, W, oh, ow;
    float fB, fx, fy, cx, cy, doffs, zmin, zmax;
    const unsigned char* color; int64_t cstep; int rgb_order;
    void* disp_out; int disp_u16; unsigned char* omask; unsigned long long* vcount;
    void* depth; int depth_u16;
    uint4* points;
    unsigned* tile_counts;                             // (batch, tiles)
    uint4* compact; unsigned long long* count;
    int vec;
};

template <bool MASKED, int BPP, bool DWORD, bool COMPACT>      // BPP 0: no colour (rgb = 0)
__global__ void __launch_bounds__(256)
disparity_to_points_kernel(const PointsArgs p) {
#pragma clang fp contract(off)
    __shared__ uint4 s_rec[COMPACT ? 1 : 1024];
    __shared__ int s_count[4];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, W = p.W, oh = p.oh, ow = p.ow;
    const int64_t plane = (int64_t)oh * ow;
    const int64_t obase = (int64_t)n * plane;
    const float* D = p.disp + (int64_t)n * H * W;
    const unsigned char* M = MASKED ? p.mask + (int64_t)n * H * W : nullptr;
    const unsigned char* C = BPP ? p.color + (int64_t)n * oh * p.cstep : nullptr;
    const float sx = (float)W / (float)ow, sy = (float)H / (float)oh, r = (float)ow / (float)W;
    const int a = p.vec ? (int)(obase & 3) : 0;
    const int64_t b0 = 4 * ((int64_t)blockIdx.x * 256) - a;                    // first element of the block's tile, image-local
    const int64_t e0 = b0 + 4 * tid;
    const int lo = e0 < 0 ? (int)-e0 : 0;
    const int hi = e0 + 4 <= plane ? 4 : (int)(plane - e0);                    // <= 0: no element (such lanes still vote below)
    const bool full = p.vec && lo == 0 && hi == 4;
    int y = 0, x = 0;
    if (lo < hi) {
        y = (int)((e0 + lo) / ow);
        x = (int)((e0 + lo) - (int64_t)y * ow);
    }
    int prefix = 0;
    if constexpr (COMPACT) {                           // ok pixels of the tiles before this one (loads issued with the gathers below)
        const unsigned* tc = p.tile_counts + (int64_t)n * gridDim.x;
        for (int i = tid; i < (int)blockIdx.x; i += 256) prefix += (int)tc[i];
    }
    float t[4][4], a1[4], b1[4], fx_[4], fy_[4];
    unsigned m[4][4], rgb[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {                      // taps and loads of all four pixels first (clamped to pixel 0 for a slot without one)
        const bool in = k >= lo && k < hi;
        const int xx = in ? x : 0, yy = in ? y : 0;
        int x0, x1, y0, y1;
        frame_tap(xx, sx, W, x0, x1, a1[k]);
        frame_tap(yy, sy, H, y0, y1, b1[k]);
        const int64_t r0 = (int64_t)y0 * W, r1 = (int64_t)y1 * W;
        t[k][0] = D[r0 + x0]; t[k][1] = D[r0 + x1]; t[k][2] = D[r1 + x0]; t[k][3] = D[r1 + x1];
        if constexpr (MASKED) {
            m[k][0] = M[r0 + x0]; m[k][1] = M[r0 + x1]; m[k][2] = M[r1 + x0]; m[k][3] = M[r1 + x1];
        }
        rgb[k] = 0u;
        if constexpr (BPP != 0) {                      // the left frame's own pixel, channels in memory order B,G,R or R,G,B; alpha dropped
            const unsigned char* px = C + (int64_t)yy * p.cstep + (int64_t)xx * BPP;
            unsigned c0, c1, c2;
            if constexpr (DWORD) {
                const unsigned q = *reinterpret_cast<const unsigned*>(px);
                c0 = q & 0xffu; c1 = (q >> 8) & 0xffu; c2 = (q >> 16) & 0xffu;
            } else {
                c0 = px[0]; c1 = px[1]; c2 = px[2];
            }
            rgb[k] = p.rgb_order ? ((c0 << 16) | (c1 << 8) | c2) : ((c2 << 16) | (c1 << 8) | c0);
        }
        fx_[k] = (float)xx; fy_[k] = (float)yy;
        if (in && ++x == ow) { x = 0; y++; }
    }
    constexpr unsigned kNaN = 0x7fc00000u;
    float dv[4], Z[4];
    unsigned valid[4], ok[4];
    uint4 rec[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool in = k >= lo && k < hi;
        const float a0 = 1.f - a1[k], bb0 = 1.f - b1[k];
        const float top = t[k][0] * a0 + t[k][1] * a1[k];
        const float bot = t[k][2] * a0 + t[k][3] * a1[k];
        float v = (top * bb0 + bot * b1[k]) * r;
        bool val = in;
        if constexpr (MASKED) {
            const int nt = (b1[k] > 0.5f ? 2 : 0) + (a1[k] > 0.5f ? 1 : 0);
            const unsigned mn = nt == 0 ? m[k][0] : (nt == 1 ? m[k][1] : (nt == 2 ? m[k][2] : m[k][3]));
            const float tn = nt == 0 ? t[k][0] : (nt == 1 ? t[k][1] : (nt == 2 ? t[k][2] : t[k][3]));
            if (!(m[k][0] && m[k][1] && m[k][2] && m[k][3])) v = tn * r;
            val = in && mn != 0;
        }
        const float den = v + p.doffs;
        bool good = val && den > 0.f && den <= 3.402823466e38f;                // (false for a NaN)
        const float z = p.fB / den;
        good = good && z >= p.zmin && z <= p.zmax;
        const float X = ((fx_[k] - p.cx) / p.fx) * z;
        const float Y = ((fy_[k] - p.cy) / p.fy) * z;
        dv[k] = v; Z[k] = z;
        valid[k] = val ? 1u : 0u;
        ok[k] = good ? 1u : 0u;
        rec[k] = good ? make_uint4(__builtin_bit_cast(unsigned, X), __builtin_bit_cast(unsigned, Y), __builtin_bit_cast(unsigned, z), rgb[k]) : make_uint4(kNaN, kNaN, kNaN, rgb[k]);
    }
    unsigned long long bal[4];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {                      // (uniform: every lane of every wave is here)
        bal[k] = __ballot(ok[k]);
        mine += __builtin_popcountll(bal[k]);
    }
    if constexpr (!COMPACT) {
        if (p.disp_out) {                              // exactly disparity_to_frame_kernel's values and stores
            if (p.disp_u16) {
                unsigned short* out = static_cast<unsigned short*>(p.disp_out) + obase;
                unsigned short ov[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float q = rintf(dv[k] * 256.f);
                    unsigned short o = (unsigned short)(q > 0.f ? (q < 65535.f ? q : 65535.f) : 0.f);      // NaN -> 0
                    if (MASKED && o == 0) o = 1;
                    ov[k] = valid[k] ? o : (unsigned short)0;
                }
                if (full) {
                    *reinterpret_cast<uint2*>(out + e0) = make_uint2((unsigned)ov[0] | ((unsigned)ov[1] << 16), (unsigned)ov[2] | ((unsigned)ov[3] << 16));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k >= lo && k < hi) out[e0 + k] = ov[k];
                }
            } else {
                float* out = static_cast<float*>(p.disp_out) + obase;
                float ov[4];
#pragma unroll
                for (int k = 0; k < 4; k++) ov[k] = valid[k] ? dv[k] : 0.f;
                if (full) {
                    *reinterpret_cast<float4*>(out + e0) = make_float4(ov[0], ov[1], ov[2], ov[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k >= lo && k < hi) out[e0 + k] = ov[k];
                }
            }
        }
        if (MASKED && p.omask) {
            unsigned char* om = p.omask + obase;
            if (full) {
                *reinterpret_cast<unsigned*>(om + e0) = (valid[0] | (valid[1] << 8) | (valid[2] << 16) | (valid[3] << 24)) * 255u;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (k >= lo && k < hi) om[e0 + k] = (unsigned char)(valid[k] * 255u);
            }
        }
        if (p.depth) {
            if (p.depth_u16) {
                unsigned short* out = static_cast<unsigned short*>(p.depth) + obase;
                unsigned short ov[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float q = rintf(Z[k] * 1000.f);
                    unsigned short o = (unsigned short)(q > 0.f ? (q < 65535.f ? q : 65535.f) : 0.f);
                    if (o == 0) o = 1;
                    ov[k] = ok[k] ? o : (unsigned short)0;
                }
                if (full) {
                    *reinterpret_cast<uint2*>(out + e0) = make_uint2((unsigned)ov[0] | ((unsigned)ov[1] << 16), (unsigned)ov[2] | ((unsigned)ov[3] << 16));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k >= lo && k < hi) out[e0 + k] = ov[k];
                }
            } else {
                unsigned* out = static_cast<unsigned*>(p.depth) + obase;
                unsigned ov[4];
#pragma unroll
                for (int k = 0; k < 4; k++) ov[k] = ok[k] ? __builtin_bit_cast(unsigned, Z[k]) : kNaN;
                if (full) {
                    *reinterpret_cast<uint4*>(out + e0) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k >= lo && k < hi) out[e0 + k] = ov[k];
                }
            }
        }
        if (p.points) {                                // (uniform: the barrier is reached by every thread or by none)
#pragma unroll
            for (int k = 0; k < 4; k++) s_rec[4 * tid + k] = rec[k];
            __syncthreads();
            uint4* P = p.points + obase;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int64_t e = b0 + 256 * j + tid;
                if (e >= 0 && e < plane) P[e] = s_rec[256 * j + tid];
            }
        }
        if (p.tile_counts || (MASKED && p.vcount)) {   // (uniform)
            int c = 0;
            if (MASKED && p.vcount) {
#pragma unroll
                for (int k = 0; k < 4; k++) c += __builtin_popcountll(__ballot(valid[k]));
            }
            if (lane == 0) s_count[wave] = p.tile_counts ? mine | (c << 12) : c;          // both at most 256 < 2^12 per wave
            __syncthreads();
            if (tid == 0) {
                if (p.tile_counts) {
                    p.tile_counts[(int64_t)n * gridDim.x + blockIdx.x] =
                        (unsigned)((s_count[0] & 0xfff) + (s_count[1] & 0xfff) + (s_count[2] & 0xfff) + (s_count[3] & 0xfff));
                    c = (s_count[0] >> 12) + (s_count[1] >> 12) + (s_count[2] >> 12) + (s_count[3] >> 12);
                } else {
                    c = s_count[0] + s_count[1] + s_count[2] + s_count[3];
                }
                if (MASKED && p.vcount && c) atomicAdd(p.vcount + n, (unsigned long long)c);               // one atomic per block
            }
        }
    } else {
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) prefix += __shfl(prefix, lane ^ s);
        __shared__ int s_prefix[4];
        if (lane == 0) { s_prefix[wave] = prefix; s_count[wave] = mine; }
        __syncthreads();
        int pos = s_prefix[0] + s_prefix[1] + s_prefix[2] + s_prefix[3];
        const int total = pos + s_count[0] + s_count[1] + s_count[2] + s_count[3];
        for (int w = 0; w < wave; w++) pos += s_count[w];
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int k = 0; k < 4; k++) pos += __builtin_popcountll(bal[k] & below);
        if (p.compact) {
            uint4* P = p.compact + obase;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (ok[k]) P[pos++] = rec[k];
        }
        if (p.count && blockIdx.x == gridDim.x - 1 && tid == 0) p.count[n] = (unsigned long long)total;
    }
}

// The viz node's 2x2 debug panel (reference ros/packages/stereo_dnn_ros_viz/src/stereo_dnn_ros_viz_node.cpp:27-130), rgb8:
//   top-left  left frame, area-resized      top-right    right frame, area-resized
//   bottom-left  disparity as grey          bottom-right disparity in the KITTI colour scheme (dispToColor, :49-79)
// One pixel of a panel packed as R | G << 8 | B << 16.
__device__ static __forceinline__ unsigned viz_sat_u8(float a) {           // saturate_cast<uchar>(cvRound(a)): nearest even, NaN -> 0
    const float v = rintf(a);
    return (unsigned)(v > 0.f ? (v < 255.f ? v : 255.f) : 0.f);
}

__device__ static __forceinline__ unsigned viz_grey(float d, float s) {    // s = 255.f / max_disp, formed once on the host
    return viz_sat_u8(d * s) * 0x010101u;
}

// cur = d / max_disp; index = the last i with cur > cumsum[i] (0 if none, also for NaN); w = (float)(1.0 - (double)((cur - cumsum[index]) *
// weights[index])), subtraction and product in fp32, each rounded on its own; channel = trunc(clamp((w * m0 + (1 - w) * m1) * 255)) in
// double, where m0 / m1 are the 0-or-1 entries of the corner colours index and index + 1: an entry of 0 contributes 0 whatever w is.
// index 7 (cur > 1) has weight 0, so w = 1 there by definition (also for an infinite cur), and the row past the table counts as 0: white.
__device__ static __forceinline__ unsigned viz_color(float d, float max_disp) {
#pragma clang fp contract(off)
    constexpr float weights[8] = {8.77192974f, 5.40540552f, 8.77192974f, 5.74712658f, 8.77192974f, 5.40540552f, 8.77192974f, 0.f};
    constexpr float cumsum[8] = {0.f, 0.114f, 0.299f, 0.413f, 0.587f, 0.70100003f, 0.88600004f, 1.f};
    const float cur = d / max_disp;
    int index = 0;
    float base = cumsum[0], wgt = weights[0];
#pragma unroll
    for (int i = 1; i < 8; i++)
        if (cur > cumsum[i]) { index = i; base = cumsum[i]; wgt = weights[i]; }
    const float x = (cur - base) * wgt;
    const double w = index == 7 ? 1.0 : (double)(float)(1.0 - (double)x);
    const double u = 1.0 - w;
    const int next = index == 7 ? 0 : index + 1;                          // w_map[i] = (i >> 1 & 1, i >> 2 & 1, i & 1); "w_map[8]" = 0
    unsigned px = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int bit = c == 0 ? 1 : (c == 1 ? 2 : 0);
        const double v = (((index >> bit) & 1 ? w : 0.0) + ((next >> bit) & 1 ? u : 0.0)) * 255.0;
        px |= (unsigned)(v > 0.0 ? (v < 255.0 ? v : 255.0) : 0.0) << (8 * c);         // a NaN or a negative value: 0
    }
    return px;
}

// The panel (MOSAIC: rows 2H x 6W bytes) or the colour picture alone (!MOSAIC: H x 3W bytes, left / right unused), one launch.
// Pixels are 3 bytes, the network widths are odd and dst_step is any number, so neither a pixel nor a panel nor a row starts on a dword.
// A block is kVizRows picture rows x 63 chunks, a chunk being an ALIGNED 12-byte piece of a row's memory: 252 pixels and the one before
// and after them, whose bytes complete the first and last chunk when the row starts off a dword.
//   phase 1: thread t forms the picture pixel 252 * blockIdx.x - 1 + t of each row -- consecutive lanes read consecutive source pixels
//            / disparities, as preprocess_frames_kernel; same area_taps, tap order and accumulation order, the x taps of the block's
//            columns and the y taps of its rows built once into LDS -- and leaves it packed in LDS;
//   phase 2: wave r stores row r: lane l takes the 4 (row on a dword: a = 0 or 3) or 5 packed pixels that overlap its chunk, shifts
//            them into three dwords and stores those.  Only a chunk cut by the row's first or last byte is stored byte by byte.
// One row per block: a thread's rows are a serial chain of dependent loads, and at the network's sizes the launch is bound by that chain
// and by the blocks' start-up (the taps), not by bytes.  Measured, 1257x369 from 1280x720 / 513x257 from 672x376 (profiles/README.md):
// 4 rows per block 19.0 / 13.6 us, 1 row 19.0 / 9.0 us, 1 row with a pixel's 9 taps loaded at once 17.0 / 7.7 us.
// The top and the bottom half of the panel are separate blocks (uniform branches).
// grid = (ceil(chunks / 63), (MOSAIC ? 2 : 1) * ceil(H / kVizRows), batch), chunks = ceil((row bytes + 3) / 12)
constexpr int kVizChunks = 63, kVizRows = 1, kVizPixels = 4 * kVizChunks + 2;
static_assert(kVizPixels + kVizRows <= 256 && kVizRows <= 4, "viz_kernel: one thread per column, the last ones build the y taps");
template <int BPP, bool DWORD, bool MOSAIC>
__global__ void __launch_bounds__(256)
viz_kernel(const unsigned char* __restrict__ left, const unsigned char* __restrict__ right, int sh, int sw, int64_t step, bool rgb_order,
           const float* __restrict__ disp, int H, int W, float max_disp, float grey_scale, unsigned char* __restrict__ dst,
           int64_t dst_step) {
    __shared__ float s_wx[kAreaMaxTaps][kVizPixels];
    __shared__ float s_wy[kVizRows][kAreaMaxTaps];
    __shared__ int s_x0[kVizPixels], s_y0[kVizRows];
    __shared__ unsigned s_px[kVizRows][kVizPixels];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int yblocks = (H + kVizRows - 1) / kVizRows;
    const bool top = MOSAIC && (int)blockIdx.y < yblocks;
    const int y0 = ((int)blockIdx.y - (MOSAIC && !top ? yblocks : 0)) * kVizRows;   // first row of the block within its panel
    const int npix = MOSAIC ? 2 * W : W;                                            // pixels of a picture row
    const int p = (int)blockIdx.x * (4 * kVizChunks) - 1 + tid;                     // picture column of this thread's pixels
    const bool second = p >= W;                                                     // right-hand panel
    const int col = second ? p - W : p;
    const bool mine = tid < kVizPixels && p >= 0 && p < npix;
    if (!mine && tid < kVizPixels)                     // a column outside the picture: its packed value is ORed beside its neighbours' below
        for (int r = 0; r < kVizRows; r++) s_px[r][tid] = 0u;
    if (top) {
        const bool resize = !(sh == H && sw == W);
        if (resize) {                                  // (uniform over the block: every thread reaches the barrier or none does)
            if (mine) {
                float wx[kAreaMaxTaps];
                s_x0[tid] = area_taps(col, (double)sw / W, sw, wx);
                for (int i = 0; i < kAreaMaxTaps; i++) s_wx[i][tid] = wx[i];
            }
            const int yt = 255 - tid;                  // the block's last threads hold no column (kVizPixels + kVizRows <= 256)
            if (yt < kVizRows && y0 + yt < H) s_y0[yt] = area_taps(y0 + yt, (double)sh / H, sh, s_wy[yt]);
            __syncthreads();
        }
        if (mine) {
            const unsigned char* s = (second ? right : left) + (int64_t)n * sh * step;
            auto pixel = [&](const unsigned char* px, unsigned& c0, unsigned& c1, unsigned& c2) {
                if constexpr (DWORD) {
                    const unsigned v = *reinterpret_cast<const unsigned*>(px);
                    c0 = v & 0xffu; c1 = (v >> 8) & 0xffu; c2 = (v >> 16) & 0xffu;
                } else {
                    c0 = px[0]; c1 = px[1]; c2 = px[2];
                }
            };
            float wx[kAreaMaxTaps];
            int x0 = 0;
            if (resize) {
                for (int i = 0; i < kAreaMaxTaps; i++) wx[i] = s_wx[i][tid];
                x0 = s_x0[tid];
            }
            for (int r = 0; r < kVizRows && y0 + r < H; r++) {
                unsigned c0, c1, c2;                                       // channels in memory order: B,G,R or R,G,B
                if (!resize) {
                    pixel(s + (int64_t)(y0 + r) * step + (int64_t)col * BPP, c0, c1, c2);
                } else if (wx[3] == 0.f && s_wy[r][3] == 0.f) {
                    // at most 3 taps an axis (every factor up to 2: the network's sizes from the usual cameras): all 9 source pixels
                    // are loaded before the first is used -- one trip to memory instead of one per source row -- at clamped
                    // addresses; a tap of weight 0 is skipped as below, so the sums are the same operations in the same order
                    const int ys = s_y0[r];
                    unsigned t[3][3][3];
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const int yy = ys + j < sh ? ys + j : sh - 1;
                        const unsigned char* row = s + (int64_t)yy * step;
#pragma unroll
                        for (int i = 0; i < 3; i++) {
                            const int xx = x0 + i < sw ? x0 + i : sw - 1;
                            pixel(row + xx * BPP, t[j][i][0], t[j][i][1], t[j][i][2]);
                        }
                    }
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const float wy = s_wy[r][j];
                        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
                        for (int i = 0; i < 3; i++) {
                            const bool on = wx[i] != 0.f;
                            r0 = on ? r0 + wx[i] * t[j][i][0] : r0; r1 = on ? r1 + wx[i] * t[j][i][1] : r1; r2 = on ? r2 + wx[i] * t[j][i][2] : r2;
                        }
                        const bool on = wy != 0.f;
                        a0 = on ? a0 + wy * r0 : a0; a1 = on ? a1 + wy * r1 : a1; a2 = on ? a2 + wy * r2 : a2;
                    }
                    c0 = viz_sat_u8(a0); c1 = viz_sat_u8(a1); c2 = viz_sat_u8(a2);
                } else {
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
                    const int ys = s_y0[r];
                    for (int j = 0; j < kAreaMaxTaps; j++) {
                        const float wy = s_wy[r][j];
                        if (wy == 0.f) continue;
                        const unsigned char* row = s + (int64_t)(ys + j) * step;
                        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
                        for (int i = 0; i < kAreaMaxTaps; i++) {
                            if (wx[i] == 0.f) continue;
                            unsigned t0, t1, t2;
                            pixel(row + (x0 + i) * BPP, t0, t1, t2);
                            r0 += wx[i] * t0; r1 += wx[i] * t1; r2 += wx[i] * t2;
                        }
                        a0 += wy * r0; a1 += wy * r1; a2 += wy * r2;
                    }
                    c0 = viz_sat_u8(a0); c1 = viz_sat_u8(a1); c2 = viz_sat_u8(a2);
                }
                s_px[r][tid] = rgb_order ? (c0 | (c1 << 8) | (c2 << 16)) : (c2 | (c1 << 8) | (c0 << 16));
            }
        }
    } else if (mine) {
        for (int r = 0; r < kVizRows && y0 + r < H; r++) {
            const float d = disp[((int64_t)n * H + (y0 + r)) * W + col];
            s_px[r][tid] = MOSAIC && !second ? viz_grey(d, grey_scale) : viz_color(d, max_disp);
        }
    }
    __syncthreads();
    const int lane = tid % 64, r = tid / 64, y = y0 + r;
    if (lane >= kVizChunks || r >= kVizRows || y >= H) return;
    unsigned char* row = dst + ((int64_t)n * (MOSAIC ? 2 * H : H) + (MOSAIC && !top ? H + y : y)) * dst_step;
    const int a = (int)(reinterpret_cast<uintptr_t>(row) & 3);                     // the row starts `a` bytes past a dword
    const int bytes = 3 * npix;
    const int b0 = 12 * ((int)blockIdx.x * kVizChunks + lane) - a;                 // row byte at which this chunk starts (< 0: the row's head)
    if (b0 >= bytes) return;
    // the chunk's bytes are bytes o .. o + 11 of the pixels 4 * chunk - (a > 0) and following; a = 0: +0, 1: +2, 2: +1, 3: +0
    const int i0 = 4 * lane + (a ? 0 : 1), o = a ? 3 - a : 0;
    const unsigned q0 = s_px[r][i0], q1 = s_px[r][i0 + 1], q2 = s_px[r][i0 + 2], q3 = s_px[r][i0 + 3];
    unsigned t[4] = {q0 | (q1 << 24), (q1 >> 8) | (q2 << 16), (q2 >> 16) | (q3 << 8), 0u};
    if (o) {                                           // (uniform over the wave)
        t[3] = s_px[r][i0 + 4];
        for (int i = 0; i < 3; i++) t[i] = (t[i] >> (8 * o)) | (t[i + 1] << (32 - 8 * o));
    }
    const int lo = b0 < 0 ? -b0 : 0, hi = bytes - b0 < 12 ? bytes - b0 : 12;      // the bytes [lo, hi) of the chunk belong to the row
    for (int i = 0; i < 3; i++) {
        if (4 * i >= lo && 4 * i + 4 <= hi) {
            *reinterpret_cast<unsigned*>(row + b0 + 4 * i) = t[i];
        } else {
            for (int j = 4 * i; j < 4 * i + 4; j++)
                if (j >= lo && j < hi) row[b0 + j] = (unsigned char)(t[i] >> (8 * (j - 4 * i)));
        }
    }
}

// out = disp * scale (in place allowed): the ROS node's `output *= w` (stereo_dnn_ros_node.cpp:81) on the device
__global__ void __launch_bounds__(256)
disparity_scale_kernel(const float* disp, float* out, int64_t n, float scale) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = disp[i] * scale;
}

__global__ void __launch_bounds__(256)
disparity_u16_kernel(const float* __restrict__ disp, unsigned short* __restrict__ out, int64_t n, float scale) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = rintf(disp[i] * scale);           // cv::saturate_cast<ushort>(cvRound(x)): nearest even
    out[i] = (unsigned short)(v < 0.f ? 0.f : (v > 65535.f ? 65535.f : v));
}

}  // namespace rt
