// resample_core.h -- the ARITHMETIC that the resamplers of wave_io.hip (one clip, a ragged batch of clips), stream_resample.hip
// (streams that arrive in chunks), band_merge.hip and stream_band.hip (two signals per output) share: resampy's running time
// register as a piecewise-linear description, and one output sample, tap for tap.  The first two call rs_output, so a stream gets
// the bits of the clip it is a prefix of; band_merge.hip and stream_band.hip call rs_output2, which keeps those bits.  What sits
// around the output loop (filter rule, grid, launch, window load, table walks) is resample_launch.h's; each table's bounds rule
// (a *_row reader and a *_why that host and kernel both call) stands in the file of its entry point.
#pragma once
#include "ragged.h"
#include <math.h>

// resampy keeps the source time of output t in a RUNNING f64 sum (time_register += 1/ratio), and because it
// walks the filter table with the truncated step int(scale * num_table), its result is not continuous where
// that time crosses an integer -- which the exact time t * 441/140 does at every 140th output of 44.1 -> 14 kHz.
// Matching it therefore needs the running sum bit for bit.  A sequential f64 sum is piecewise linear: while the
// register and register + inc share a binade [2^e, 2^(e+1)) every addition rounds on the same grid and adds the
// same d = rn_grid(inc).  The host builds that piecewise description (a few entries per binade: one explicit
// step across each binade boundary, one where a round-to-even tie settles, then a run) and the kernel evaluates
// time(t) = fma(t - k0, d, s0) exactly.
#define RS_MAXSEG 120
struct RsSegs {
    int n;
    long long k0[RS_MAXSEG];
    double s0[RS_MAXSEG], d[RS_MAXSEG];
};

// The description of the outputs 0 .. n_out - 1; with `stop`, it ends earlier, as soon as the register has reached `stop`
// (sos_stream_resample_ready: the first output whose time is not below a sample count).  k_end: the first output the
// description does not cover.  -1: more than RS_MAXSEG segments.
static int rs_build_segments(double inc, long long n_out, RsSegs* g, double stop = INFINITY, long long* k_end = nullptr) {
    long long k = 0;
    double s = 0.0;
    g->n = 0;
    while (k < n_out && s < stop) {
        if (g->n == RS_MAXSEG) return -1;
        const int i = g->n++;
        volatile double s1v = s + inc;                   // one literal step of the running sum
        const double s1 = s1v;
        g->k0[i] = k; g->s0[i] = s; g->d[i] = s1 - s;
        int e;
        const double limit = s > 0.0 ? ldexp(1.0, (frexp(s, &e), e)) : 0.0;      // top of s's binade
        volatile double s2v = s1 + inc;
        const double s2 = s2v;
        if (!(s > 0.0) || !(s2 < limit) || (s2 - s1) != (s1 - s)) { k += 1; s = s1; continue; }   // explicit single step
        const double d = s1 - s;
        // largest M with s + M*d + inc < limit: steps k .. k+M+1 all add d
        long long M = (long long)((limit - inc - s) / d);
        if (M < 1) M = 1;
        for (;;) { volatile double v = fma((double)M, d, s) + inc; if (v < limit || M == 1) break; --M; }
        for (;;) { volatile double v = fma((double)(M + 1), d, s) + inc; if (!(v < limit)) break; ++M; }
        k += M + 1;
        s = fma((double)(M + 1), d, s);
    }
    if (k_end) *k_end = k;
    return 0;
}

// time(t) of the description, for 0 <= t within what it covers
__host__ __device__ static inline double rs_time(const RsSegs& seg, int64_t t) {
    int sg = seg.n - 1;
    while (sg > 0 && seg.k0[sg] > t) --sg;
    return fma((double)(t - seg.k0[sg]), seg.d[sg], seg.s0[sg]);
}

// Where rs_output finds sample p of its signal.  RsLinear: at x[p], a clip that lies in one piece.  RsRing: at
// ring[p % cap], a stream in its ring (stream_window.hip).  at(p) -> a cursor, prev / next move it by one sample.
struct RsLinear {
    const float* x;
    __device__ __forceinline__ int64_t at(int64_t p) const { return p; }
    __device__ __forceinline__ int64_t prev(int64_t c) const { return c - 1; }
    __device__ __forceinline__ int64_t next(int64_t c) const { return c + 1; }
    __device__ __forceinline__ float load(int64_t c) const { return x[c]; }
};
struct RsRing {
    const float* ring;
    int64_t cap;
    __device__ __forceinline__ int64_t at(int64_t p) const { return p % cap; }        // p >= 0
    __device__ __forceinline__ int64_t prev(int64_t c) const { return c == 0 ? cap - 1 : c - 1; }
    __device__ __forceinline__ int64_t next(int64_t c) const { return c + 1 == cap ? 0 : c + 1; }
    __device__ __forceinline__ float load(int64_t c) const { return ring[c]; }
};

// win: half window already scaled by min(1, ratio), nwin entries.  Output t:
//   time = resampy's running sum (RsSegs); n = floor(time); frac = scale * (time - n)
//   left wing : sum_i (w[o + i*step] + eta * (w[o + i*step + 1] - w[o + i*step])) * x[n - i],    o = int(frac * num_table)
//   right wing: the same with frac' = scale - frac over x[n + 1 + k]
// where the difference table has a zero last entry (resampy: interp_delta[-1] = 0): LDS holds w[nwin] = w[nwin-1].
// One output sample of one signal of n_in samples, found through `src`; w = the window in LDS.  Every kernel calls this, so
// a signal gets the same bits from each.  Neither wing reads more than nwin / index_step samples.
template <typename Src>
__device__ __forceinline__ float rs_output(const Src& src, int64_t n_in, const RsSegs& seg, double scale, const float* w, int nwin,
                                           int num_table, int index_step, int64_t t) {
    const double time = rs_time(seg, t);
    const int64_t n = (int64_t)time;
    double frac = scale * (time - (double)n);
    double index_frac = frac * (double)num_table;
    int o = (int)index_frac;
    float eta = (float)(index_frac - (double)o);
    float acc = 0.f;
    {
        const int64_t lim = (int64_t)((nwin - o) / index_step);
        const int i_max = (int)(n + 1 < lim ? n + 1 : lim);
        int64_t c = src.at(n);
        for (int i = 0; i < i_max; ++i, o += index_step, c = src.prev(c)) {
            const float a = w[o], b = w[o + 1];
            acc = fmaf(fmaf(eta, b - a, a), src.load(c), acc);
        }
    }
    frac = scale - frac;
    index_frac = frac * (double)num_table;
    o = (int)index_frac;
    eta = (float)(index_frac - (double)o);
    {
        const int64_t lim = (int64_t)((nwin - o) / index_step);
        const int64_t rem = n_in - n - 1;
        const int k_max = (int)(rem < lim ? rem : lim);
        if (k_max > 0) {
            int64_t c = src.at(n + 1);
            for (int k = 0; k < k_max; ++k, o += index_step, c = src.next(c)) {
                const float a = w[o], b = w[o + 1];
                acc = fmaf(fmaf(eta, b - a, a), src.load(c), acc);
            }
        }
    }
    return acc;
}

// rs_output of TWO signals that share the time register (band_merge.hip: the 14 kHz input of the networks and their output,
// back at the recording's rate; stream_band.hip: the same two out of their rings): *ya = rs_output(sa, na, ..., t) and *yb =
// rs_output(sb, nb, ..., t) bit for bit, nb <= na, with every tap weight formed once.  The weights depend on t alone, so each
// sum sees rs_output's taps in rs_output's order with the same fmaf nesting; the two differ in where the right wing ends
// (n_in - n - 1), and each ends at its own.  b_live: whether output t of sb is resampled at all (t < its n_valid); *yb = 0
// otherwise, and also if the time of t lies at or past sb's end (no tap of sb is read then).
template <typename SrcA, typename SrcB>
__device__ __forceinline__ void rs_output2(const SrcA& sa, int64_t na, const SrcB& sb, int64_t nb, bool b_live, const RsSegs& seg,
                                           double scale, const float* w, int nwin, int num_table, int index_step, int64_t t,
                                           float* ya, float* yb) {
    const double time = rs_time(seg, t);
    const int64_t n = (int64_t)time;
    *ya = 0.f;
    *yb = 0.f;
    if (n >= na) return;                  // never for t < (int64)(na * ratio); no read past a signal's end in any case
    b_live = b_live && n < nb;
    double frac = scale * (time - (double)n);
    double index_frac = frac * (double)num_table;
    int o = (int)index_frac;
    float eta = (float)(index_frac - (double)o);
    float acc_a = 0.f, acc_b = 0.f;
    {
        const int64_t lim = (int64_t)((nwin - o) / index_step);
        const int i_max = (int)(n + 1 < lim ? n + 1 : lim);
        int64_t ca = sa.at(n);
        if (b_live) {
            int64_t cb = sb.at(n);
            for (int i = 0; i < i_max; ++i, o += index_step, ca = sa.prev(ca), cb = sb.prev(cb)) {
                const float a = w[o], b = w[o + 1];
                const float wt = fmaf(eta, b - a, a);
                acc_a = fmaf(wt, sa.load(ca), acc_a);
                acc_b = fmaf(wt, sb.load(cb), acc_b);
            }
        } else {
            for (int i = 0; i < i_max; ++i, o += index_step, ca = sa.prev(ca)) {
                const float a = w[o], b = w[o + 1];
                acc_a = fmaf(fmaf(eta, b - a, a), sa.load(ca), acc_a);
            }
        }
    }
    frac = scale - frac;
    index_frac = frac * (double)num_table;
    o = (int)index_frac;
    eta = (float)(index_frac - (double)o);
    {
        const int64_t lim = (int64_t)((nwin - o) / index_step);
        const int64_t rem_a = na - n - 1, rem_b = b_live ? nb - n - 1 : 0;
        const int ka_max = (int)(rem_a < lim ? rem_a : lim);
        const int kb_max = (int)(rem_b < lim ? rem_b : lim);      // <= ka_max: nb <= na
        if (ka_max > 0) {
            int64_t ca = sa.at(n + 1);
            int k = 0;
            if (kb_max > 0) {
                int64_t cb = sb.at(n + 1);
                for (; k < kb_max; ++k, o += index_step, ca = sa.next(ca), cb = sb.next(cb)) {
                    const float a = w[o], b = w[o + 1];
                    const float wt = fmaf(eta, b - a, a);
                    acc_a = fmaf(wt, sa.load(ca), acc_a);
                    acc_b = fmaf(wt, sb.load(cb), acc_b);
                }
            }
            for (; k < ka_max; ++k, o += index_step, ca = sa.next(ca)) {
                const float a = w[o], b = w[o + 1];
                acc_a = fmaf(fmaf(eta, b - a, a), sa.load(ca), acc_a);
            }
        }
    }
    *ya = acc_a;
    *yb = acc_b;
}
