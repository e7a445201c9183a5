// band_core.h -- the gains arithmetic that band_merge.hip (whole clips) and stream_band.hip (streams in their rings) share, so a
// live stream gets the bits of the file it is a prefix of: the ratio r[j] of one hop frame, the mean s[j] of r around a frame,
// the frame-centre position p of a native sample and the interpolation g[t] of s at p.  Float64 restatement:
// tests/band_reference.py; the streaming rule on top of it: tests/stream_band_reference.py.
#pragma once
#include "resample_core.h"

#define BG_MAX_SMOOTH 16        // K <= 16 frames of smoothing on each side

// r of the frame that covers the low-rate samples [s0, s1) of a (found through sa) and of b (through sb, reading zero from mp
// on): E_a = sum a^2, E_b = sum b^2 in f64, lane-strided fma sums of ONE wave (all 64 lanes call this) folded by a __shfl_down
// tree; r = 1 if E_a == 0 else min(1, sqrt(E_b / E_a)).  The value is lane 0's.
template <typename SrcA, typename SrcB>
__device__ __forceinline__ double band_frame_ratio(const SrcA& sa, const SrcB& sb, int64_t s0, int64_t s1, int64_t mp, int lane) {
    double ea = 0.0, eb = 0.0;
    for (int64_t i = s0 + lane; i < s1; i += 64) {
        const double va = (double)sa.load(sa.at(i));
        ea = fma(va, va, ea);
        if (i < mp) {
            const double vb = (double)sb.load(sb.at(i));
            eb = fma(vb, vb, eb);
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        ea += __shfl_down(ea, d, 64);
        eb += __shfl_down(eb, d, 64);
    }
    return ea == 0.0 ? 1.0 : fmin(1.0, sqrt(eb / ea));
}

// Where band_mean finds r[q].  BandRTile: a tile in LDS that starts at frame lo.  BandRRing: ring[q % cap], a stream's frames.
struct BandRTile {
    const double* r;
    int64_t lo;
    __device__ __forceinline__ double get(int64_t q) const { return r[q - lo]; }
};
struct BandRRing {
    const double* ring;
    int64_t cap;
    __device__ __forceinline__ double get(int64_t q) const { return ring[q % cap]; }       // q >= 0
};

// s[j] = the ascending f64 mean of r[max(0, j - K) .. j + K], cut at J - 1 where J is known (J < 0: the stream is still open,
// and the caller asks only for frames whose r[j + K] exists), stored as f32
template <typename R>
__device__ __forceinline__ float band_mean(const R& r, int64_t j, int K, int64_t J) {
    const int64_t w0 = j - K > 0 ? j - K : 0, w1 = (J < 0 || j + K < J - 1) ? j + K : J - 1;
    double sum = 0.0;
    for (int64_t q = w0; q <= w1; ++q) sum += r.get(q);
    return (float)(sum / (double)(w1 - w0 + 1));
}

// The frame-centre position of native sample t, frame = ratio * hop native samples per hop of the low rate.  The kernels and
// the host's count of final outputs (sos_stream_band_ready) evaluate this one expression.
__host__ __device__ static inline double band_gain_pos(int64_t t, double frame) { return ((double)t + 0.5) / frame - 0.5; }

// The last frame of s that g[t] reads while no end clamps it: 0 for p <= 0, floor(p) + 1 otherwise
__host__ __device__ static inline int64_t band_gain_last(double p) { return !(p > 0.0) ? 0 : (int64_t)p + 1; }

// g[t]: s interpolated linearly at p, s[0] for p <= 0 and s[J - 1] for p >= J - 1 (J < 0: no end is known, none clamps);
// evaluated in f64 and rounded to f32.  s(j) -> s[j] as f32.
template <typename S>
__device__ __forceinline__ float band_gain_at(const S& s, double p, int64_t J) {
    if (!(p > 0.0)) return s(0);
    if (J >= 0 && p >= (double)(J - 1)) return s(J - 1);
    const int64_t i = (int64_t)p;
    const double s_lo = (double)s(i), s_hi = (double)s(i + 1);
    return (float)(s_lo + (p - (double)i) * (s_hi - s_lo));
}
