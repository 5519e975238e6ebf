// What a camera really puts into image_raw -> the colour frames the frame path takes: mono8 / mono16, the four 8-bit Bayer mosaics
// (bilinear demosaicing, mosaic reflected about its edge samples) and YUV 4:2:2 as UYVY or YUYV (integer BT.601, limited range).
// include/rt_stereo.h carries the full statement (rt_decode_frames_u8); everything here is 32-bit integer arithmetic.
#pragma once
#include "common.hip.h"
#include "imgproc.hip.h"

namespace rt {

enum { kDecodeMono8 = 0, kDecodeMono16 = 1, kDecodeBayer = 2, kDecodeYuv = 3 };
constexpr int kDecodeRun = 4;                // pixels a lane decodes in a row: one dword of mono8 / Bayer, two of mono16 / YUV

struct DecodeArgs {
    const unsigned char *left, *right;       // wire frames: h x w pixels, rows `step` bytes apart, frame n at n * h * step
    unsigned char *dleft, *dright;           // decoded frames, 3 or 4 bytes a pixel: rows dstep bytes apart
    int h, w;
    int64_t step, dstep;
    int batch;
    int rgb;                                 // byte 0 of a decoded pixel is R (rgb8 / rgba8), else B
    int r_row, r_col;                        // Bayer: (y & 1, x & 1) of the R sites; B sits on the other diagonal end
    int yuy2;                                // YUV: Y0 U Y1 V, else U Y0 V Y1
};

// N dwords at a 4-byte aligned address, as one access
template <int N>
__device__ static __forceinline__ void decode_load_dwords(const unsigned char* p, unsigned (&d)[N]) {
    __builtin_memcpy(d, __builtin_assume_aligned(p, 4), 4 * N);
}
// bytes [0, nbytes) at any address, packed little-endian; the rest 0
template <int N>
__device__ static __forceinline__ void decode_load_bytes(const unsigned char* p, int nbytes, unsigned (&d)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) d[i] = 0u;
#pragma unroll
    for (int i = 0; i < 4 * N; i++)
        if (i < nbytes) d[i / 4] |= (unsigned)p[i] << (8 * (i % 4));
}

__device__ static __forceinline__ unsigned decode_pixel(int r, int g, int b, int rgb) {
    return 0xff000000u | ((unsigned)g << 8) | (rgb ? (unsigned)r | ((unsigned)b << 16) : (unsigned)b | ((unsigned)r << 16));
}

__device__ static __forceinline__ int decode_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// cvtColor(COLOR_YUV2BGR_UYVY)'s fixed-point BT.601: 20 fractional bits, >> is arithmetic
__device__ static __forceinline__ unsigned decode_yuv(int Y, int U, int V, int rgb) {
    constexpr int CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527;
    const int y = (Y > 16 ? Y - 16 : 0) * CY + (1 << 19), u = U - 128, v = V - 128;
    return decode_pixel(decode_clamp255((y + CVR * v) >> 20), decode_clamp255((y + CVG * v + CUG * u) >> 20), decode_clamp255((y + CUB * u) >> 20),
                        rgb);
}

// index i in [-1, n] of an axis of n >= 2 samples, reflected about the edge samples (BORDER_REFLECT_101); a larger i counts as n
__device__ static __forceinline__ int decode_reflect(int i, int n) {
    i = i > n ? n : i;
    return i < 0 ? -i : i > n - 1 ? 2 * (n - 1) - i : i;
}

// Mosaic columns x0 - 1 .. x0 + 4 of one row, byte k in bits 8k.  `full` (the run lies in the row, the row starts on a dword): the run as
// one dword, its two neighbours as bytes; otherwise six bytes, of which those past the row's reflected end are never used.
__device__ static __forceinline__ unsigned long long decode_bayer_row(const unsigned char* row, int x0, int w, bool full) {
    if (full) {
        unsigned m[1];
        decode_load_dwords(row + x0, m);
        const unsigned lo = row[x0 > 0 ? x0 - 1 : 1], hi = row[x0 + 4 < w ? x0 + 4 : w - 2];
        return (unsigned long long)lo | ((unsigned long long)m[0] << 8) | ((unsigned long long)hi << 40);
    }
    unsigned long long v = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) v |= (unsigned long long)row[decode_reflect(x0 - 1 + k, w)] << (8 * k);
    return v;
}

// npix <= 4 pixels (byte c of px[i] is byte c of pixel i) to p.  ALIGNED and a whole run: 12 or 16 contiguous bytes as dwords.
template <int BPP, bool ALIGNED>
__device__ static __forceinline__ void decode_store_run(unsigned char* p, const unsigned (&px)[kDecodeRun], int npix) {
    if (ALIGNED && npix == kDecodeRun) {
        if constexpr (BPP == 4) {
            __builtin_memcpy(__builtin_assume_aligned(p, 4), px, 16);
        } else {
            const unsigned d[3] = {(px[0] & 0xffffffu) | (px[1] << 24), ((px[1] >> 8) & 0xffffu) | (px[2] << 16), ((px[2] >> 16) & 0xffu) | (px[3] << 8)};
            __builtin_memcpy(__builtin_assume_aligned(p, 4), d, 12);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < kDecodeRun; i++)
        if (i < npix) {
#pragma unroll
            for (int c = 0; c < BPP; c++) p[i * BPP + c] = (unsigned char)(px[i] >> (8 * c));
        }
}

// Both frames of a pair batch, wire encoding in, 3 or 4 bytes a pixel out.  A block is 256 columns x 4 rows (8 for a mosaic): one wave a
// row, each lane a run of 4 pixels, so a wave reads 256 (mono8, Bayer) or 512 contiguous bytes and writes 768 or 1024 contiguous bytes.
// ALIGNED (every base and step a multiple of 4): a whole run is loaded as one or two dwords in one access and stored as three or four;
// the run cut by the row's end, and every run when !ALIGNED, goes byte by byte and touches nothing outside its pixels.
// A mosaic lane makes two rows of its run from four mosaic rows (y0 - 1 .. y0 + 2, y0 even), each read once as a dword plus the byte on
// either side, instead of three rows for every output row.
// grid = (ceil(w / 256), ceil(h / 4) or ceil(h / 8), 2 * batch): z < batch -> left frame z, else right frame z - batch
template <int MODE, int BPP, bool ALIGNED>
__global__ void __launch_bounds__(256)
decode_frames_kernel(DecodeArgs a) {
    constexpr int ROWS = MODE == kDecodeBayer ? 2 : 1;
    const int tx = threadIdx.x % kFramesCols, ty = threadIdx.x / kFramesCols;
    const int x0 = ((int)blockIdx.x * kFramesCols + tx) * kDecodeRun;
    const int y0 = ((int)blockIdx.y * kFramesRows + ty) * ROWS;
    if (x0 >= a.w || y0 >= a.h) return;
    const bool second = (int)blockIdx.z >= a.batch;
    const int n = second ? blockIdx.z - a.batch : blockIdx.z;
    const unsigned char* s = (second ? a.right : a.left) + (int64_t)n * a.h * a.step;
    unsigned char* d = (second ? a.dright : a.dleft) + ((int64_t)n * a.h + y0) * a.dstep + (int64_t)x0 * BPP;
    const int npix = a.w - x0 < kDecodeRun ? a.w - x0 : kDecodeRun;
    const bool full = ALIGNED && npix == kDecodeRun;
    unsigned px[kDecodeRun];
    if constexpr (MODE == kDecodeMono8) {
        const unsigned char* p = s + (int64_t)y0 * a.step + x0;
        unsigned v[1];
        if (full) decode_load_dwords(p, v);
        else decode_load_bytes(p, npix, v);
#pragma unroll
        for (int i = 0; i < kDecodeRun; i++) px[i] = 0xff000000u | (((v[0] >> (8 * i)) & 0xffu) * 0x010101u);
        decode_store_run<BPP, ALIGNED>(d, px, npix);
    } else if constexpr (MODE == kDecodeMono16 || MODE == kDecodeYuv) {
        const unsigned char* p = s + (int64_t)y0 * a.step + (int64_t)x0 * 2;
        unsigned v[2];
        if (full) decode_load_dwords(p, v);
        else decode_load_bytes(p, 2 * npix, v);
        if constexpr (MODE == kDecodeMono16) {
#pragma unroll
            for (int i = 0; i < kDecodeRun; i++) {
                const unsigned v16 = (v[i / 2] >> (16 * (i % 2))) & 0xffffu;           // little-endian
                const unsigned g = (v16 + 127u + ((v16 >> 8) & 1u)) >> 8;               // rint(v16 / 256), ties to even
                px[i] = 0xff000000u | ((g > 255u ? 255u : g) * 0x010101u);
            }
        } else {
#pragma unroll
            for (int j = 0; j < kDecodeRun / 2; j++) {
                const int b0 = v[j] & 0xffu, b1 = (v[j] >> 8) & 0xffu, b2 = (v[j] >> 16) & 0xffu, b3 = v[j] >> 24;
                const int U = a.yuy2 ? b1 : b0, V = a.yuy2 ? b3 : b2;
                px[2 * j] = decode_yuv(a.yuy2 ? b0 : b1, U, V, a.rgb);
                px[2 * j + 1] = decode_yuv(a.yuy2 ? b2 : b3, U, V, a.rgb);
            }
        }
        decode_store_run<BPP, ALIGNED>(d, px, npix);
    } else {
        unsigned long long m[ROWS + 2];
#pragma unroll
        for (int k = 0; k < ROWS + 2; k++) m[k] = decode_bayer_row(s + (int64_t)decode_reflect(y0 - 1 + k, a.h) * a.step, x0, a.w, full);
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            if (y0 + r >= a.h) break;
            const unsigned long long up = m[r], c = m[r + 1], dn = m[r + 2];
            const bool on_r_row = r == a.r_row;                                     // (y0 is even: the row's phase is r)
#pragma unroll
            for (int i = 0; i < kDecodeRun; i++) {
                const auto at = [i](unsigned long long row, int k) { return (int)((row >> (8 * (i + 1 + k))) & 0xffu); };
                const int site = at(c, 0), hs = at(c, -1) + at(c, 1), vs = at(up, 0) + at(dn, 0);
                const bool on_r_col = (i & 1) == a.r_col;                           // (x0 is a multiple of 4: the column's phase is i & 1)
                int R, G, B;
                if (on_r_row == on_r_col) {                                         // an R or a B site
                    const int other = (at(up, -1) + at(up, 1) + at(dn, -1) + at(dn, 1) + 2) >> 2;
                    G = (hs + vs + 2) >> 2;
                    R = on_r_row ? site : other;
                    B = on_r_row ? other : site;
                } else {                                                            // a G site: R lies beside it in an R row, else above and below
                    const int hc = (hs + 1) >> 1, vc = (vs + 1) >> 1;
                    G = site;
                    R = on_r_row ? hc : vc;
                    B = on_r_row ? vc : hc;
                }
                px[i] = decode_pixel(R, G, B, a.rgb);
            }
            decode_store_run<BPP, ALIGNED>(d + (int64_t)r * a.dstep, px, npix);
        }
    }
}

}  // namespace rt
