// ragged.h -- what the three ragged-batch measures (metrics_batch.hip, stoi.hip, sdr.hip) share: the clip-count check, the
// workspace layout arithmetic, the clamped grid, the bounds rule of their plan kernels and the 256-thread LDS reductions.
// A batch is two concatenated signals plus a device table [offsets, lengths]; the host sizes every array from its own copy
// of the lengths (lengths_host), the kernels follow the device table.
#pragma once
#include "sos_common.h"
#include <algorithm>

#define MT 256                          // threads per workgroup of the block reductions below
#define RAGGED_MAX_CLIPS 65535          // clips per launch sequence: the kernels' grid.y

static inline bool ragged_clips_ok(const int64_t* lengths, int nclips) {
    return lengths && nclips > 0 && nclips <= RAGGED_MAX_CLIPS;
}

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// workspace layout: take(bytes) returns the offset of the next array and moves on to the next 256-byte boundary
struct RaggedBump {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t at = o;
        o = align256(o + bytes);
        return at;
    }
};

// ceil(units / per_block) workgroups, at least 1, at most cap (the kernels stride over what the grid does not cover)
static inline unsigned ragged_grid(int64_t units, int per_block, int64_t cap) {
    return (unsigned)std::min<int64_t>(std::max<int64_t>((units + per_block - 1) / per_block, 1), cap);
}

// The bounds rule of every plan kernel: a clip [off, off + n) of the device table is followed only if it lies inside the
// `total` samples the host summed from lengths_host (what both signals are known to hold); otherwise the clip gets status
// -1, extents 0 and no work.  No overflowing add.
__host__ __device__ static inline bool ragged_clip_inside(int64_t off, int64_t n, int64_t total) {
    return off >= 0 && n >= 0 && n <= total && off <= total - n;
}

// Reductions over the MT threads of a workgroup through LDS (red: f64 [MT], scan: int [MT]), fixed trees.  block_sum and
// block_max return the same bits on every thread and leave `red` free for the next call.
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = MT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ static inline double block_max(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = MT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// inclusive scan of one int per thread; returns this thread's inclusive value (scan[MT - 1] is the total until the caller's
// next barrier)
__device__ static inline int block_scan_incl(int v, int* scan) {
    scan[threadIdx.x] = v;
    __syncthreads();
    for (int s = 1; s < MT; s <<= 1) {
        const int u = (int)threadIdx.x >= s ? scan[threadIdx.x - s] : 0;
        __syncthreads();
        scan[threadIdx.x] += u;
        __syncthreads();
    }
    return scan[threadIdx.x];
}
