// resample_launch.h -- what sits AROUND the output loop of the five resampling entry points, each piece written once:
// sos_resample_f32 and sos_resample_batch_f32 (wave_io.hip), sos_resample_merge_batch_f32 (band_merge.hip),
// sos_stream_resample_f32 (stream_resample.hip), sos_stream_band_merge_f32 (stream_band.hip) and the host-only counts
// sos_stream_resample_ready / sos_stream_band_ready.  The arithmetic of an output is resample_core.h's.
//   host    rs_filter (the filter rule), rs_segments / rs_row_segments (the time register), rs_grid (one workgroup per CU),
//           rs_launch (the dynamic-LDS limit once per device, then the launch), rs_rings / RsSlotsOnce (the ring arguments)
//   device  rs_load_window, rs_clip_of_tile (column tables with a first-tile column)
// Every kernel here keeps the whole half window in LDS, which leaves room for ONE workgroup per CU.
#pragma once
#include "resample_core.h"
#include <vector>

#define RS_LDS_MAX (160 * 1024)         // bytes of LDS a workgroup may ask for

// ---------------------------------------------------------------------------------------------- host
// What a ratio and a filter table give: scale = min(1, ratio), the step through the table, the samples R a wing reads at
// most and the bytes of the window in LDS (its nwin entries and the copy of the last one, see rs_load_window).
struct RsFilter { double scale; int index_step; int64_t reach; size_t lds; };

// The filter rule of every entry point; false with the error set.  launch: the window goes into LDS, so it has at least two
// entries and fits; the *_ready counts run no kernel and take any window of at least one entry.
static bool rs_filter(const char* who, double ratio, int nwin, int num_table, bool launch, RsFilter* f) {
    if (!(ratio > 0.0) || nwin < (launch ? 2 : 1) || num_table < 1) {
        sos_set_error("%s: bad args (ratio=%g, nwin=%d, num_table=%d)", who, ratio, nwin, num_table);
        return false;
    }
    f->lds = ((size_t)nwin + 1) * sizeof(float);
    if (launch && f->lds > RS_LDS_MAX) {
        sos_set_error("%s: nwin=%d: (nwin + 1) * 4 bytes must fit the 160 KB LDS", who, nwin);
        return false;
    }
    f->scale = ratio < 1.0 ? ratio : 1.0;
    f->index_step = (int)(f->scale * (double)num_table);
    if (f->index_step < 1) {
        sos_set_error("%s: ratio %g too small for a %d-point table", who, ratio, num_table);
        return false;
    }
    f->reach = nwin / f->index_step;
    return true;
}

// rs_build_segments at a ratio; SOS_ENOSPC with the error set if the description does not fit the kernel argument
static int rs_segments(const char* who, double ratio, int64_t n_out, RsSegs* g, double stop = INFINITY, long long* k_end = nullptr) {
    if (rs_build_segments(1.0 / ratio, n_out, g, stop, k_end) == 0) return SOS_OK;
    sos_set_error("%s: time register of %lld outputs needs more than %d segments", who, (long long)n_out, RS_MAXSEG);
    return SOS_ENOSPC;
}

// The time register of a row table, t_hi(r) = the last output + 1 of host row r: every stream starts at 0, so one description,
// up to the largest t_hi (*max_t, at least 1), serves all rows.  SOS_EINVAL names a row that ends past 2^52.
template <typename THi>
static int rs_row_segments(const char* who, int nrows, const THi& t_hi_of, double ratio, RsSegs* g, int64_t* max_t) {
    *max_t = 1;
    for (int r = 0; r < nrows; ++r) {
        const int64_t t_hi = t_hi_of(r);
        if (t_hi > (int64_t)1 << 52) { sos_set_error("%s: row %d ends at output %lld", who, r, (long long)t_hi); return SOS_EINVAL; }
        *max_t = std::max(*max_t, t_hi);
    }
    return rs_segments(who, ratio, *max_t, g);
}

// The grid of a kernel that walks total_tiles >= 1 tiles gridDim.x apart: one workgroup per CU, or one per tile where there
// are fewer.  0 with the error set if the device does not tell its CUs.
static unsigned rs_grid(const char* who, int64_t total_tiles) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 1) {
        sos_set_error("%s: cannot read the number of compute units", who);
        return 0;
    }
    return (unsigned)(total_tiles < cus ? total_tiles : cus);
}

// Launches Kernel with `lds` bytes of dynamic LDS, having raised its limit once per device (one flag per kernel instance).
template <auto Kernel, typename... Args>
static int rs_launch(const char* who, unsigned grid, unsigned threads, size_t lds, sos_stream_t stream, const Args&... args) {
    static sos_device_once attr_once;
    if (sos_per_device_once(attr_once, [who] {
            if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_MAX) != hipSuccess) {
                sos_set_error("%s: cannot raise the dynamic LDS limit", who);
                return (int)SOS_ELAUNCH;
            }
            return (int)SOS_OK;
        }))
        return SOS_ELAUNCH;
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), lds, (hipStream_t)stream, args...);
    return sos_check_launch(who);
}

// The ring arguments of a stream entry point: a table of nrows rows over `slots` streams, each with per_slot rings of cap
// samples (stream_window.hip's layout: ring row * cap, at most RAGGED_MAX_CLIPS rows); false with the error set.
static bool rs_rings(const char* who, int nrows, int64_t slots, int per_slot, int64_t cap) {
    if (nrows < 1 || nrows > RAGGED_MAX_CLIPS || slots < 1 || slots > RAGGED_MAX_CLIPS / per_slot || cap < 1 ||
        cap > INT64_MAX / 8 / RAGGED_MAX_CLIPS) {
        sos_set_error("%s: bad args (1 .. 65535 rows, got %d; 1 .. %d slots, got %lld; rings of %lld samples)", who, nrows,
                      RAGGED_MAX_CLIPS / per_slot, (long long)slots, (long long)cap);
        return false;
    }
    return true;
}

// A table names a slot once: two rows of one launch would write one stream's outputs in no order.
struct RsSlotsOnce {
    std::vector<uint8_t> seen;
    explicit RsSlotsOnce(int64_t slots) : seen(slots, 0) {}
    // row r names `slot` (inside the slots); false with the error set if an earlier row did
    bool take(const char* who, int r, int64_t slot) {
        if (seen[slot]) {
            sos_set_error("%s: row %d names slot %lld, which an earlier row of the table names", who, r, (long long)slot);
            return false;
        }
        seen[slot] = 1;
        return true;
    }
};

// ---------------------------------------------------------------------------------------------- device
// w[0 .. nwin] in LDS = the half window and, as entry nwin, its last entry again: the zero last difference of rs_output
template <int THREADS>
__device__ __forceinline__ void rs_load_window(float* w, const float* __restrict__ win, int nwin) {
    for (int i = threadIdx.x; i <= nwin; i += THREADS) w[i] = win[i < nwin ? i : nwin - 1];
    __syncthreads();
}

// Column tables: the last clip whose first tile (tile0[c], ascending from 0) is <= tile
__device__ __forceinline__ int rs_clip_of_tile(const int64_t* __restrict__ tile0, int nclips, int64_t tile) {
    int lo = 0, hi = nclips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile0[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}
