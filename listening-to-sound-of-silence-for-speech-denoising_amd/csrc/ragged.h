// ragged.h -- what every ragged-batch entry point shares (metrics_batch.hip, stoi.hip, sdr.hip, ragged_io.hip,
// silence_label.hip, ragged_mix.hip, wave_io.hip, ragged_window.hip, band_merge.hip): the clip-count check, the clip row, the bounds rule on
// both sides of the launch, the host's sums over a table, the workspace layout arithmetic, the clamped grid, the 256-thread LDS
// reductions and the four-sample accesses of clips that start on any sample.
// A batch is clips back to back in one buffer plus a table of where each lies, in two copies: the host sizes every array
// from its own (table_host / lengths_host) and refuses a bad entry before any launch; the kernels follow the DEVICE table.
// A table with more columns than the clip row below states its rule once, next to its kernel, as a *_row reader and a
// __host__ __device__ *_why that the kernel's skip and the host's refusal both call (loudness_core.h: ld_row; limiter.hip: lim_row; wave_io.hip:
// rs_batch_why; band_merge.hip: band_gain_why, band_merge_why; stream_resample.hip and stream_band.hip: their stream_*_why).
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

// The bounds rule: a clip [off, off + n) of the device table is followed only if it lies inside the `total` elements the
// host summed from its own table (what the buffers are known to hold); otherwise the clip gets no work (and, where the
// kernel reports one, status -1).  No overflowing add.
__host__ __device__ static inline bool ragged_clip_inside(int64_t off, int64_t n, int64_t total) {
    return off >= 0 && n >= 0 && n <= total && off <= total - n;
}

// The clip row of sos_ragged_stage_f32 and sos_silence_label_batch: int64 [nclips][4]
#define RAGGED_CLIP_COLS 4
struct RaggedClip { int64_t off, n, foff, frames; };      // sample offset, samples, frame offset, frames
__host__ __device__ static inline RaggedClip ragged_clip(const int64_t* table, int64_t b) {
    const int64_t* te = table + b * RAGGED_CLIP_COLS;
    return {te[0], te[1], te[2], te[3]};
}
// the device rule for such a row: both extents lie inside (total samples, total frames)
__host__ __device__ static inline bool ragged_row_inside(const RaggedClip& c, int64_t total, int64_t total_frames) {
    return ragged_clip_inside(c.off, c.n, total) && ragged_clip_inside(c.foff, c.frames, total_frames);
}

// Host: adds column `col` of a row-major table [nrows][cols] to `s` from row `first` on, every entry within [lo, hi] and the
// sum within INT64_MAX / 8 (bytes of f64 stay inside int64); returns nrows, or the first entry it cannot accept.
struct RaggedSum { int64_t total = 0, longest = 0; };
static inline int ragged_sum_column(const int64_t* table, int nrows, int cols, int col, int64_t lo, int64_t hi, RaggedSum* s,
                                    int first = 0) {
    for (int r = first; r < nrows; ++r) {
        const int64_t v = table[(int64_t)r * cols + col];
        if (v < lo || v > hi || v > INT64_MAX / 8 - s->total) return r;
        s->total += v;
        s->longest = std::max(s->longest, v);
    }
    return nrows;
}
// Host: nrows, or the index of the first entry whose [table[off_col], + table[len_col]) leaves the `total` elements
static inline int ragged_first_outside(const int64_t* table, int nrows, int cols, int off_col, int len_col, int64_t total) {
    for (int r = 0; r < nrows; ++r)
        if (!ragged_clip_inside(table[(int64_t)r * cols + off_col], table[(int64_t)r * cols + len_col], total)) return r;
    return nrows;
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

// Four consecutive samples of a clip that may start on any sample (ragged_io.hip, ragged_mix.hip, ragged_window.hip): one
// 16-byte access where the address allows it, sample by sample otherwise.  Which of the two is taken changes no value.
typedef float ragged_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bool ragged_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }      // a null pointer counts

// v = p[j0 .. j0 + 4): one 16-byte load if `vec` (p + j0 aligned, all four inside), else the samples below `end` one by one
__device__ __forceinline__ void ragged_load4(const float* p, int64_t j0, int64_t end, bool vec, float (&v)[4]) {
    if (vec) {
        const ragged_f32x4 q = *(const ragged_f32x4*)(p + j0);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + k < end) v[k] = p[j0 + k];
    }
}
// p[j0 .. j0 + 4) = v, likewise
__device__ __forceinline__ void ragged_store4(float* p, int64_t j0, int64_t end, bool vec, const float (&v)[4]) {
    if (vec) {
        *(ragged_f32x4*)(p + j0) = ragged_f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + k < end) p[j0 + k] = v[k];
    }
}
