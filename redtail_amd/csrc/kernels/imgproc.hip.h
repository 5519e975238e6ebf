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
