// mask_rule.h -- the bits -> sample-mask rule (M2/tools.py:340-362, convert_bitstreammask_to_audiomask) as device functions,
// shared by bits_to_mask_kernel (frontend.hip: rectangular and padded batches) and ragged_stage_kernel (ragged_io.hip: clips
// back to back, one ratio per clip).  One statement of the arithmetic: both kernels give the same bits for the same clip.
#pragma once
#include "sos_common.h"

// The frame edge, int(i * ratio) as Python's float64 evaluates it: ONE rounded multiply (the host is compiled with
// -ffp-contract=on: the volatile product keeps it out of an fma).  The mask rule below and silence_label.hip both use it.
__host__ __device__ __forceinline__ int64_t frame_edge(int64_t i, double ratio) {
#ifdef __HIP_DEVICE_COMPILE__
    return (int64_t)__dmul_rn((double)i, ratio);
#else
    volatile double p = (double)i * ratio;
    return (int64_t)p;
#endif
}

// The frame decision (M1/predict.py:117-119): sigmoid of a logit in f32.  bit = frame_sigmoid(x) >= threshold, 1 = non-silent.
// The ONE statement of it: threshold_kernel (frontend.hip) and window_frames_link_kernel (ragged_window.hip) give the same
// bits for the same logit.
__device__ __forceinline__ float frame_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ uint8_t frame_decision(float x, float thr) { return frame_sigmoid(x) >= thr ? 1 : 0; }

// Pre-flip mask value of sample j: 1 if j lies in [int(i*r), int((i+1)*r - 1)) of a silent
// frame i (bit 0), else 0.  All index arithmetic in IEEE double with explicit (un-fused)
// multiply/add so it reproduces Python's float64 evaluation bit for bit.
__device__ __forceinline__ int premask(const uint8_t* bits, int64_t n_frames, double ratio, int64_t j) {
    int64_t i0 = (int64_t)((double)j / ratio);
    for (int64_t i = i0 - 1; i <= i0 + 1; ++i) {
        if (i < 0 || i >= n_frames) continue;
        const int64_t lo = frame_edge(i, ratio);
        const int64_t hi = (int64_t)__dadd_rn(__dmul_rn((double)(i + 1), ratio), -1.0);
        if (j >= lo && j < hi) return bits[i] == 0 ? 1 : 0;
    }
    return 0;
}

// Mask value (1 on silent samples) of sample j of a clip of n_samples samples and n_frames frame decisions `bits`
// (1 = non-silent): premask, with every ORIGINAL run shorter than five samples flipped.
__device__ __forceinline__ float mask_sample(const uint8_t* __restrict__ bits, int64_t n_frames, double ratio, int64_t n_samples,
                                             int64_t j) {
    if (ratio >= 16.0) {
        // Frames are longer than the 9-sample neighbourhood: j - 4 .. j + 4 can only lie in the frames i0 - 1 .. i0 + 1 of
        // sample j, whose [lo, hi) are computed ONCE (same un-fused double arithmetic as premask, so the values are the
        // same bit for bit); the per-neighbour double division + three interval evaluations made this kernel ALU bound
        // (37 us for 64 clips against ~5 us of HBM time).
        const int64_t i0 = (int64_t)((double)j / ratio);
        int64_t lo[3], hi[3];
        int val[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int64_t i = i0 - 1 + q;
            const bool ok = i >= 0 && i < n_frames;
            lo[q] = ok ? frame_edge(i, ratio) : 0;
            hi[q] = ok ? (int64_t)__dadd_rn(__dmul_rn((double)(i + 1), ratio), -1.0) : 0;      // empty interval when !ok
            val[q] = ok && bits[i] == 0 ? 1 : 0;
        }
        auto pm = [&](const int64_t jj) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (jj >= lo[q] && jj < hi[q]) return val[q];
            return 0;
        };
        const int v = pm(j);
        int len = 1;
        for (int d = 1; d <= 4 && j - d >= 0; ++d) {
            if (pm(j - d) != v) break;
            ++len;
        }
        for (int d = 1; d <= 4 && j + d < n_samples && len < 5; ++d) {
            if (pm(j + d) != v) break;
            ++len;
        }
        return (float)(len < 5 ? 1 - v : v);
    }
    const int v = premask(bits, n_frames, ratio, j);
    // length of the ORIGINAL run containing j (capped): the reference flips every run shorter
    // than 5 samples in one pass over the original runs (groupby never sees its own writes).
    int len = 1;
    for (int d = 1; d <= 4 && j - d >= 0; ++d) {
        if (premask(bits, n_frames, ratio, j - d) != v) break;
        ++len;
    }
    for (int d = 1; d <= 4 && j + d < n_samples && len < 5; ++d) {
        if (premask(bits, n_frames, ratio, j + d) != v) break;
        ++len;
    }
    return (float)(len < 5 ? 1 - v : v);
}
