// Speckle filter of a disparity map (stereo_image_proc's speckle_size / speckle_range, cv::filterSpeckles): connected components of the
// live pixels under 4-neighbour adjacency |d(p) - d(q)| <= max_diff, components of at most max_size pixels are removed.
// include/rt_stereo.h carries the full statement (rt_disparity_speckle).
//
// Labelling: a union-find forest in an array with the invariant label[i] <= i (a pixel's index inside its image; a parent is never behind
// its child), so the root of a tree is the smallest index of its component, every walk towards a root strictly decreases an integer, and
// a link is made by an atomic min of the larger root's word to the smaller root.  Four ordinary launches, each a kernel boundary:
//   speckle_tile_kernel    32 x 32 tiles in LDS: runs along the rows first, then the columns; writes per pixel the image index of its
//                          tile-local root (dead pixels: kSpeckleDead) and, at every tile-local root, the component's pixel count in the tile
//   speckle_border_kernel  one thread per pixel pair across a tile border: the lock-free union in global memory
//   speckle_size_kernel    every tile-local root that is not its component's root adds its count to the root's: one add per tile-local
//                          component, none per pixel
//   speckle_apply_kernel   keep = live and size[root] > max_size; output, mask, and the count with one atomic per block
// Workgroups never wait for one another.  Inside a launch they meet only in the border kernel, and only through agent-scope atomics
// (loads included: an XCD's L2 is not coherent with another's for plain loads); there a stale value is an older ancestor of the same
// tree, which the retry loop of the union absorbs.  Everything else one launch reads was written by an earlier launch.  The result does
// not depend on the order in which anything ran: the components are a property of the image, and their sizes are integer sums.
#pragma once
#include "common.hip.h"

namespace rt {

constexpr int kSpeckleTile = 32;                       // tile edge: 1024 pixels, 4 consecutive pixels of a row per thread
constexpr unsigned kSpeckleDead = 0xffffffffu;

// The words workgroups (global memory, agent scope) or the waves of one workgroup (LDS, workgroup scope) share while links are made.
// The emulator runs one fiber at a time: plain read-modify-write is atomic there.
#ifdef HIPEMU
template <bool GLOBAL>
struct SpeckleWord {
    static unsigned load(const unsigned* p) { return *p; }
    static unsigned fetch_min(unsigned* p, unsigned v) { const unsigned o = *p; if (v < o) *p = v; return o; }
    static unsigned fetch_add(unsigned* p, unsigned v) { const unsigned o = *p; *p = o + v; return o; }
};
#else
template <bool GLOBAL>
struct SpeckleWord {
    static constexpr int kScope = GLOBAL ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP;
    __device__ static __forceinline__ unsigned load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, kScope); }
    __device__ static __forceinline__ unsigned fetch_min(unsigned* p, unsigned v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, kScope); }
    __device__ static __forceinline__ unsigned fetch_add(unsigned* p, unsigned v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, kScope); }
};
#endif

// root of x: label[i] <= i, so x strictly decreases until it stands still
template <typename WORD>
__device__ static __forceinline__ unsigned speckle_find(const unsigned* label, unsigned x) {
    for (;;) {
        const unsigned p = WORD::load(label + x);
        if (p >= x) return x;                          // (p == x; a word above its index cannot exist, and would end the walk here)
        x = p;
    }
}
// the same where no link is made any more (an earlier launch, or an earlier phase behind a barrier, wrote every word)
__device__ static __forceinline__ unsigned speckle_find_plain(const unsigned* label, unsigned x) {
    for (;;) {
        const unsigned p = label[x];
        if (p >= x) return x;
        x = p;
    }
}

// Lock-free union: find both roots, atomic-min the larger root's word to the smaller root; if the word was no root any more, what it
// held is an ancestor that has to join the smaller root instead: go on from there.  a + b strictly decreases from pass to pass.
template <typename WORD>
__device__ static __forceinline__ void speckle_unite(unsigned* label, unsigned a, unsigned b) {
    for (;;) {
        a = speckle_find<WORD>(label, a);
        b = speckle_find<WORD>(label, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = WORD::fetch_min(label + a, b);
        if (old == a) return;
        a = old;
    }
}

__device__ static __forceinline__ bool speckle_adjacent(float a, float b, float max_diff) {
#pragma clang fp contract(off)
    return fabsf(a - b) <= max_diff;                   // (a NaN -- a dead pixel in LDS -- and inf - inf compare false)
}

// (a) tiles in LDS.  grid = (tiles_x * tiles_y, batch), 256 threads: thread t owns columns 4 (t % 8) .. + 3 of tile row t / 8.
__global__ void __launch_bounds__(256)
speckle_tile_kernel(const float* disp, const unsigned char* mask, int H, int W, int tiles_x, float max_diff, unsigned* label, unsigned* size) {
    constexpr int T = kSpeckleTile;
    __shared__ unsigned s_val[T * T];                  // the pixel's bits, a NaN where it is not live; later the tile-local counts
    __shared__ unsigned s_label[T * T];
    typedef SpeckleWord<false> LDS;
    const int tid = threadIdx.x;
    const int ly = tid >> 3, lx0 = (tid & 7) * 4;
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * T + ly, x0 = (int)(blockIdx.x % (unsigned)tiles_x) * T + lx0;
    const int64_t plane = (int64_t)H * W, base = (int64_t)blockIdx.y * plane;
    const unsigned l0 = (unsigned)(ly * T + lx0);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = __builtin_nanf("");
        if (y < H && x0 + k < W) {
            const int64_t g = base + (int64_t)y * W + x0 + k;
            const float d = disp[g];
            if (!mask || mask[g] != 0) v[k] = d;       // (a NaN disparity stays a NaN: not live)
        }
    }
    // runs along the row inside the thread's four pixels: a pixel adjacent to its left neighbour takes that neighbour's label
    unsigned lab[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        lab[k] = k > 0 && speckle_adjacent(v[k - 1], v[k], max_diff) ? lab[k - 1] : l0 + k;
        s_val[l0 + k] = __builtin_bit_cast(unsigned, v[k]);
        s_label[l0 + k] = v[k] == v[k] ? lab[k] : kSpeckleDead;
    }
    __syncthreads();
    // the run across the thread's left edge, then the columns.  A column link is skipped where the square it closes already has its
    // other three sides: (k-1, k), (up k-1, up k) and (up k-1, k-1) adjacent means k reaches `up k` without this link.
    if (lx0 > 0 && speckle_adjacent(__builtin_bit_cast(float, s_val[l0 - 1]), v[0], max_diff)) speckle_unite<LDS>(s_label, l0, l0 - 1);
    if (ly > 0) {
        float up[4];
#pragma unroll
        for (int k = 0; k < 4; k++) up[k] = __builtin_bit_cast(float, s_val[l0 + k - T]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!speckle_adjacent(up[k], v[k], max_diff)) continue;
            if (k > 0 && speckle_adjacent(v[k - 1], v[k], max_diff) && speckle_adjacent(up[k - 1], up[k], max_diff) &&
                speckle_adjacent(up[k - 1], v[k - 1], max_diff))
                continue;
            speckle_unite<LDS>(s_label, l0 + k, l0 + k - T);
        }
    }
    __syncthreads();
    // every link is made: roots by plain reads, counts into the LDS the values no longer need
    unsigned* s_count = s_val;
    unsigned root[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        root[k] = v[k] == v[k] ? speckle_find_plain(s_label, l0 + k) : kSpeckleDead;
        s_count[l0 + k] = 0;
    }
    __syncthreads();
    {                                                  // one add per stretch of equal roots
        unsigned r = kSpeckleDead, c = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (root[k] != r) {
                if (c) LDS::fetch_add(s_count + r, c);
                r = root[k];
                c = 0;
            }
            c += r != kSpeckleDead;
        }
        if (c) LDS::fetch_add(s_count + r, c);
    }
    __syncthreads();
    // a tile is row-major like the image, so the order of two of its pixels is the same in both: label[i] <= i carries over
    const int ty = y - ly, tx = x0 - lx0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (y >= H || x0 + k >= W) continue;
        const int64_t g = base + (int64_t)y * W + x0 + k;
        const unsigned r = root[k];
        label[g] = r == kSpeckleDead ? kSpeckleDead : (unsigned)((int64_t)(ty + (int)(r / T)) * W + tx + (int)(r % T));
        size[g] = r == l0 + k ? s_count[r] : 0u;
    }
}

// (b) tile borders in global memory.  Item i < nv: row i % H of the vertical border in front of column 32 (1 + i / H), the pair (x - 1, x);
// the others: column j % W of the horizontal border in front of row 32 (1 + j / W), the pair (y - 1, y).  grid = (ceil(items / 256), batch)
__global__ void __launch_bounds__(256)
speckle_border_kernel(const float* disp, const unsigned char* mask, int H, int W, int64_t nv, int64_t items, float max_diff, unsigned* label) {
    typedef SpeckleWord<true> GLB;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int64_t plane = (int64_t)H * W, base = (int64_t)blockIdx.y * plane;
    int64_t p, q;                                      // q in front of p
    if (i < nv) {
        p = (i % H) * W + (1 + i / H) * kSpeckleTile;
        q = p - 1;
    } else {
        const int64_t j = i - nv;
        p = (1 + j / W) * kSpeckleTile * (int64_t)W + j % W;
        q = p - W;
    }
    if (mask && (mask[base + p] == 0 || mask[base + q] == 0)) return;
    if (!speckle_adjacent(disp[base + p], disp[base + q], max_diff)) return;
    speckle_unite<GLB>(label + base, (unsigned)p, (unsigned)q);
}

// (c) sizes from the tile level up.  grid = (ceil(H W / 256), batch)
__global__ void __launch_bounds__(256)
speckle_size_kernel(const unsigned* label, unsigned* size, int64_t plane) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= plane) return;
    const int64_t base = (int64_t)blockIdx.y * plane;
    if (label[base + i] >= (unsigned)i) return;        // dead, or a root: nothing to hand up (only roots are added to, only others are read)
    const unsigned c = size[base + i];
    if (c == 0) return;                                // not a tile-local root
    const unsigned r = speckle_find_plain(label + base, (unsigned)i);
    SpeckleWord<true>::fetch_add(size + base + r, c);
}

// (d) apply and count.  FILTER = false (max_size == 0): keep = live, no labels.  out may be disp, out_mask may be mask: a thread reads its
// own pixel before it writes it.  grid = (ceil(H W / 256), batch)
template <bool FILTER>
__global__ void __launch_bounds__(256)
speckle_apply_kernel(const float* disp, const unsigned char* mask, int64_t plane, unsigned max_size, const unsigned* label, const unsigned* size,
                     float* out, unsigned char* out_mask, unsigned long long* count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t base = (int64_t)blockIdx.y * plane;
    bool keep = false;
    if (i < plane) {
        const float d = disp[base + i];
        keep = (!mask || mask[base + i] != 0) && d == d;
        if (FILTER && keep) keep = size[base + speckle_find_plain(label + base, (unsigned)i)] > max_size;
        out[base + i] = keep ? d : 0.f;
        if (out_mask) out_mask[base + i] = keep ? 255 : 0;
    }
    if (count) {                                       // (uniform: every lane of every wave is still here)
        __shared__ int s_count[4];
        const int c = __builtin_popcountll(__ballot(keep));
        if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int t = s_count[0] + s_count[1] + s_count[2] + s_count[3];
            if (t) atomicAdd(count + blockIdx.y, (unsigned long long)t);                             // one atomic per block
        }
    }
}

}  // namespace rt
