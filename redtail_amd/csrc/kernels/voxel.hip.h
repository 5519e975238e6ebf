// Voxel-grid downsampling of a PointXYZRGB cloud (pcl::VoxelGrid behind stereo_image_proc/point_cloud2): one record per occupied cell, the
// centroid of its points and their mean colour, in ascending cell index.  include/rt_stereo.h carries the full statement
// (rt_points_voxel_grid).
//
// Order without a sort: the cells that hold a point are marked in a bitmap (one bit per cell), the popcounts of its words are scanned,
// and the RANK of an occupied cell -- prefix[word] + popcount(bits below) -- is its slot: ranks ascend with the cell by construction.
// Ordinary launches, each a kernel boundary (the clear of the bitmap in front is a memset):
//   voxel_mark_kernel        a lane takes kVoxelRun consecutive records and ORs their cells' bits into the bitmap, one atomic per stretch
//                            of records that share a word
//   voxel_scan_kernel        exclusive scan inside blocks of kVoxelScan elements + the blocks' sums (over bitmap words: popcounts;
//                            over slots, with min_points > 1: N >= min_points)
//   voxel_scan_sums_kernel   one workgroup per image: exclusive scan of the blocks' sums in place, the total beside them.  The kernels
//                            behind fold the block's offset in: rank = sums[block] + prefix[word] + popcount(bits below)
//   voxel_zero_kernel        zeroes the accumulators of the occupied slots (their number came out of the scan)
//   voxel_accumulate_kernel  every point recomputes its cell, looks up its rank and adds into its slot: five 64-bit adds per stretch of
//                            records that share a cell
//   voxel_emit_kernel        a thread per bitmap word: every set bit's slot -> centroid, colour, record at its output index
// Workgroups never wait for one another.  Inside a launch they meet only in mark and accumulate, and only through relaxed agent-scope
// atomics without a return value: an OR of bits and sums of integers, whose results do not depend on the order of arrival.  Everything
// else a launch reads, an earlier launch wrote.  The output therefore is a function of the SET of points of an image.
#pragma once
#include "common.hip.h"

namespace rt {

constexpr int kVoxelRun = 4;                           // consecutive records per lane in mark and accumulate
constexpr int kVoxelScan = 1024;                       // elements per scan block: 256 threads x 4
constexpr unsigned kVoxelNone = 0xffffffffu;           // the cell of a record outside the grid (cells < 2^27)
constexpr int kVoxelAcc = 5;                           // 64-bit words per slot: N | R << 32, G | B << 32, S_x, S_y, S_z

struct VoxelArgs {
    float o[3], leaf[3];
    int dims[3];
    int capacity;                                      // records per image of the input
    int64_t words;                                     // bitmap words per image = ceil(cells / 32)
    int64_t slots;                                     // accumulator slots per image = min(capacity, cells)
    int scan_blocks;                                   // blocks of the word scan per image = ceil(words / kVoxelScan)
    int slot_blocks;                                   // blocks of the slot scan per image = ceil(slots / kVoxelScan)
};

// What workgroups share while a launch runs.  The emulator runs one fiber at a time: plain read-modify-write is atomic there.
#ifdef HIPEMU
struct VoxelShared {
    static void fetch_or(unsigned* p, unsigned v) { *p |= v; }
    static void add(unsigned long long* p, unsigned long long v) { *p += v; }
};
#else
struct VoxelShared {
    __device__ static __forceinline__ void fetch_or(unsigned* p, unsigned v) {
        (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ static __forceinline__ void add(unsigned long long* p, unsigned long long v) {
        (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
#endif

// cell of a record and the 16-bit offsets inside it; kVoxelNone when the point is outside the grid (a NaN fails every comparison)
__device__ static __forceinline__ unsigned voxel_cell(const VoxelArgs& a, const uint4& rec, unsigned q[3]) {
#pragma clang fp contract(off)
    unsigned cell = 0;
    bool in = true;
    const unsigned bits[3] = {rec.x, rec.y, rec.z};
    int idx[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float t = (__builtin_bit_cast(float, bits[k]) - a.o[k]) / a.leaf[k];
        in = in && t >= 0.f && t < (float)a.dims[k];
        const float fl = floorf(t);
        idx[k] = in ? (int)fl : 0;
        const float f = t - fl;
        q[k] = in ? (unsigned)(f * 65536.f) : 0u;
    }
    cell = (unsigned)((idx[2] * a.dims[1] + idx[1]) * a.dims[0] + idx[0]);
    return in ? cell : kVoxelNone;
}

// records of image n that are read: all of them, or the first min(count[n], capacity)
__device__ static __forceinline__ int64_t voxel_records(const VoxelArgs& a, const unsigned long long* count, int n) {
    if (!count) return a.capacity;
    const unsigned long long c = count[n];
    return c < (unsigned long long)a.capacity ? (int64_t)c : (int64_t)a.capacity;
}

// (a) mark.  grid = (ceil(capacity / (256 kVoxelRun)), batch)
__global__ void __launch_bounds__(256)
voxel_mark_kernel(VoxelArgs a, const uint4* points, const unsigned long long* count, unsigned* bitmap) {
    const int n = blockIdx.y;
    const int64_t records = voxel_records(a, count, n);
    const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * kVoxelRun;
    if (first >= records) return;
    const uint4* src = points + (int64_t)n * a.capacity;
    unsigned* bm = bitmap + (int64_t)n * a.words;
    unsigned word = kVoxelNone, mask = 0;              // the stretch in hand
#pragma unroll
    for (int k = 0; k < kVoxelRun; k++) {
        if (first + k >= records) break;
        unsigned q[3];
        const unsigned cell = voxel_cell(a, src[first + k], q);
        if (cell == kVoxelNone) continue;
        if ((cell >> 5) != word) {
            if (mask) VoxelShared::fetch_or(bm + word, mask);
            word = cell >> 5;
            mask = 0;
        }
        mask |= 1u << (cell & 31);
    }
    if (mask) VoxelShared::fetch_or(bm + word, mask);
}

// exclusive scan of one value per thread over the 256 threads of a workgroup (s: 256 words of LDS); returns the prefix, *total the sum
__device__ static __forceinline__ unsigned voxel_block_scan(unsigned v, unsigned* s, unsigned* total) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned t = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    const unsigned incl = s[tid];
    *total = s[255];
    __syncthreads();                                   // (s may be written again by the caller's next round)
    return incl - v;
}

// (b) scan inside blocks.  SLOTS = false: element i is popcount(bitmap word i), i < words.  SLOTS = true: element k is
// N(slot k) >= min_points, k < occupied (totals[2 n]).  prefix[i] = sum of the block's elements in front of i; sums[block] = the block's sum.
// grid = (scan_blocks or slot_blocks, batch)
template <bool SLOTS>
__global__ void __launch_bounds__(256)
voxel_scan_kernel(VoxelArgs a, const unsigned* bitmap, const unsigned long long* acc, const unsigned* totals, unsigned min_points,
                  unsigned* prefix, unsigned* sums) {
    __shared__ unsigned s_scan[256];
    const int n = blockIdx.y;
    const int64_t per_image = SLOTS ? a.slots : a.words;
    const int64_t limit = SLOTS ? (int64_t)totals[2 * n] : a.words;
    const int64_t i0 = (int64_t)blockIdx.x * kVoxelScan + threadIdx.x * 4;
    unsigned v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = 0;
        if (i0 + k < limit && i0 + k < per_image) {
            if (SLOTS) v[k] = (unsigned)(acc[((int64_t)n * a.slots + i0 + k) * kVoxelAcc] & 0xffffffffull) >= min_points ? 1u : 0u;
            else v[k] = (unsigned)__builtin_popcount(bitmap[(int64_t)n * a.words + i0 + k]);
        }
        sum += v[k];
    }
    unsigned total;
    unsigned run = voxel_block_scan(sum, s_scan, &total);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (i0 + k < per_image && i0 + k < limit) prefix[(int64_t)n * per_image + i0 + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) sums[(int64_t)n * (SLOTS ? a.slot_blocks : a.scan_blocks) + blockIdx.x] = total;
}

// (c) scan of the blocks' sums, in place, and the image's total to *(totals + 2 n + which).  grid = (batch), one workgroup per image
__global__ void __launch_bounds__(256)
voxel_scan_sums_kernel(unsigned* sums, int blocks, unsigned* totals, int which) {
    __shared__ unsigned s_scan[256];
    const int n = blockIdx.x;
    unsigned* s = sums + (int64_t)n * blocks;
    unsigned carry = 0;
    for (int base = 0; base < blocks; base += 256) {   // (uniform: every thread makes every round)
        const int i = base + (int)threadIdx.x;
        const unsigned v = i < blocks ? s[i] : 0u;
        unsigned total;
        const unsigned pre = voxel_block_scan(v, s_scan, &total);
        if (i < blocks) s[i] = carry + pre;
        carry += total;
    }
    if (threadIdx.x == 0) totals[2 * n + which] = carry;
}

// (d) zero the accumulators of the occupied slots.  grid = (ceil(slots kVoxelAcc / 256), batch)
__global__ void __launch_bounds__(256)
voxel_zero_kernel(VoxelArgs a, const unsigned* totals, unsigned long long* acc) {
    const int n = blockIdx.y;
    int64_t occupied = totals[2 * n];
    if (occupied > a.slots) occupied = a.slots;        // (cannot be: every occupied cell holds one of at most `capacity` points)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < occupied * kVoxelAcc) acc[(int64_t)n * a.slots * kVoxelAcc + i] = 0ull;
}

// rank of an occupied cell
__device__ static __forceinline__ int64_t voxel_rank(const unsigned* bm, const unsigned* prefix, const unsigned* sums, unsigned cell) {
    const unsigned w = cell >> 5;
    return (int64_t)sums[w / kVoxelScan] + prefix[w] + (unsigned)__builtin_popcount(bm[w] & ((1u << (cell & 31)) - 1u));
}

// (e) accumulate.  grid = (ceil(capacity / (256 kVoxelRun)), batch)
__global__ void __launch_bounds__(256)
voxel_accumulate_kernel(VoxelArgs a, const uint4* points, const unsigned long long* count, const unsigned* bitmap, const unsigned* prefix,
                        const unsigned* sums, unsigned long long* acc) {
    const int n = blockIdx.y;
    const int64_t records = voxel_records(a, count, n);
    const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * kVoxelRun;
    if (first >= records) return;
    const uint4* src = points + (int64_t)n * a.capacity;
    const unsigned* bm = bitmap + (int64_t)n * a.words;
    const unsigned* pre = prefix + (int64_t)n * a.words;
    const unsigned* blk = sums + (int64_t)n * a.scan_blocks;
    unsigned long long* dst = acc + (int64_t)n * a.slots * kVoxelAcc;
    unsigned cur = kVoxelNone;                         // the stretch in hand: its cell and its five sums
    unsigned long long s0 = 0, s1 = 0, sx = 0, sy = 0, sz = 0;
    auto flush = [&]() {
        if (cur == kVoxelNone) return;
        const int64_t slot = voxel_rank(bm, pre, blk, cur);
        if (slot >= a.slots) return;                   // (cannot be: mark set this cell's bit from the same record)
        unsigned long long* p = dst + slot * kVoxelAcc;
        VoxelShared::add(p + 0, s0);
        VoxelShared::add(p + 1, s1);
        VoxelShared::add(p + 2, sx);
        VoxelShared::add(p + 3, sy);
        VoxelShared::add(p + 4, sz);
    };
#pragma unroll
    for (int k = 0; k < kVoxelRun; k++) {
        if (first + k >= records) break;
        const uint4 rec = src[first + k];
        unsigned q[3];
        const unsigned cell = voxel_cell(a, rec, q);
        if (cell == kVoxelNone) continue;
        if (cell != cur) {
            flush();
            cur = cell;
            s0 = s1 = sx = sy = sz = 0;
        }
        s0 += 1ull | ((unsigned long long)((rec.w >> 16) & 255u) << 32);
        s1 += (unsigned long long)((rec.w >> 8) & 255u) | ((unsigned long long)(rec.w & 255u) << 32);
        sx += q[0];
        sy += q[1];
        sz += q[2];
    }
    flush();
}

// (f) emit.  A thread per bitmap word.  FILTER = false (min_points == 1): slot k is record k, the image's number is totals[2 n].
// FILTER = true: record index = slot_sums[k / kVoxelScan] + slot_prefix[k] for the slots with N >= min_points, the number totals[2 n + 1].
// grid = (ceil(words / 256), batch)
template <bool FILTER>
__global__ void __launch_bounds__(256)
voxel_emit_kernel(VoxelArgs a, const unsigned* bitmap, const unsigned* prefix, const unsigned* sums, const unsigned long long* acc,
                  const unsigned* slot_prefix, const unsigned* slot_sums, const unsigned* totals, unsigned min_points, uint4* voxels,
                  int out_capacity, unsigned long long* out_count, unsigned* out_cell, unsigned* out_n) {
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w == 0) out_count[n] = totals[2 * n + (FILTER ? 1 : 0)];
    if (w >= a.words) return;
    unsigned bits = bitmap[(int64_t)n * a.words + w];
    if (bits == 0) return;
    int64_t slot = (int64_t)sums[(int64_t)n * a.scan_blocks + w / kVoxelScan] + prefix[(int64_t)n * a.words + w];
    const unsigned long long* src = acc + (int64_t)n * a.slots * kVoxelAcc;
    for (; bits != 0; bits &= bits - 1, slot++) {
        if (slot >= a.slots) return;                   // (cannot be, see voxel_zero_kernel)
        const unsigned long long* p = src + slot * kVoxelAcc;
        const unsigned long long w0 = p[0];
        const unsigned N = (unsigned)(w0 & 0xffffffffull);
        int64_t rec = slot;
        if (N == 0) continue;                          // (cannot be: a set bit is a cell with a point)
        if (FILTER) {
            if (N < min_points) continue;
            rec = (int64_t)slot_sums[(int64_t)n * a.slot_blocks + slot / kVoxelScan] + slot_prefix[(int64_t)n * a.slots + slot];
        }
        if (rec >= out_capacity) continue;
        const unsigned long long w1 = p[1];
        const unsigned cell = (unsigned)(w << 5) + (unsigned)__builtin_ctz(bits);
        const unsigned xy = (unsigned)(a.dims[0] * a.dims[1]);
        const int idx[3] = {(int)(cell % (unsigned)a.dims[0]), (int)(cell % xy / (unsigned)a.dims[0]), (int)(cell / xy)};
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double g = ((double)p[2 + k] / (double)N + 0.5) / 65536.0;
            const float corner = a.o[k] + (float)idx[k] * a.leaf[k];
            c[k] = corner + (float)g * a.leaf[k];
        }
        const unsigned half = N / 2;
        const unsigned r = ((unsigned)(w0 >> 32) + half) / N, g8 = ((unsigned)(w1 & 0xffffffffull) + half) / N, b = ((unsigned)(w1 >> 32) + half) / N;
        const int64_t o = (int64_t)n * out_capacity + rec;
        voxels[o] = make_uint4(__builtin_bit_cast(unsigned, c[0]), __builtin_bit_cast(unsigned, c[1]), __builtin_bit_cast(unsigned, c[2]),
                               r << 16 | g8 << 8 | b);
        if (out_cell) out_cell[o] = cell;
        if (out_n) out_n[o] = N;
    }
}

}  // namespace rt
