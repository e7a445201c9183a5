// metrics_frame.h -- the per-frame arithmetic of the objective measures (frame energies, LLR, WSS), one copy for the
// one-clip kernels (metrics.hip) and the ragged-batch kernels (metrics_batch.hip).  Every function is called by a whole
// workgroup of MT threads on ONE frame (`ref` / `deg` point at the frame's first sample) and keeps the order of operations
// of the round-1 kernels, so both callers return the same bits for the same frame.  LDS is handed in by the caller.
// Frames: `winlength` samples under w[i] = 0.5 (1 - cos(2 pi (i+1) / (winlength+1))) (`window`, f64).
#pragma once
#include "ragged.h"                  // MT, block_sum / block_max / block_scan_incl

#define LLR_MAXP 16
#define WSS_NCRIT 25

// sa = sum (w c)^2, sb = sum (w c - w p)^2 (on every thread); red: f64 [MT]
__device__ __forceinline__ void metric_frame_energy(const float* __restrict__ ref, const float* __restrict__ deg, int winlength,
                                                    const double* __restrict__ window, double* red, double& sa, double& sb) {
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < winlength; i += MT) {
        const double c = (double)ref[i] * window[i], p = (double)deg[i] * window[i];
        a += c * c; b += (c - p) * (c - p);
    }
    sa = block_sum(a, red);
    sb = block_sum(b, red);
}

// LLR of the frame: autocorrelation lags 0..P of both windowed frames (f64), Levinson-Durbin (lane 0), then -- like the
// reference, which casts R and the LPC vectors to float32 first -- the two quadratic forms in f32.  Thread 0 writes *out.
// fr: f64 [2][winlength], red: f64 [MT], R: f64 [2][LLR_MAXP + 1]
__device__ __forceinline__ void metric_frame_llr(const float* __restrict__ ref, const float* __restrict__ deg, int winlength,
                                                 const double* __restrict__ window, int P, double* fr, double* red,
                                                 double (*R)[LLR_MAXP + 1], float* __restrict__ out) {
    for (int i = threadIdx.x; i < winlength; i += MT) {
        fr[i] = (double)ref[i] * window[i];
        fr[winlength + i] = (double)deg[i] * window[i];
    }
    __syncthreads();
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k <= P; ++k) {
            double a = 0;
            for (int i = threadIdx.x; i < winlength - k; i += MT) a += fr[s * winlength + i] * fr[s * winlength + i + k];
            const double v = block_sum(a, red);
            if (threadIdx.x == 0) R[s][k] = v;
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        float A[2][LLR_MAXP + 1];
        for (int s = 0; s < 2; ++s) {
            double a[LLR_MAXP], ap[LLR_MAXP], E = R[s][0];
            for (int i = 0; i < P; ++i) a[i] = 1.0;
            for (int i = 0; i < P; ++i) {
                double sum = 0;
                for (int j = 0; j < i; ++j) { ap[j] = a[j]; sum += a[j] * R[s][i - j]; }
                const double rc = (R[s][i + 1] - sum) / E;
                a[i] = rc;
                for (int j = 0; j < i; ++j) a[j] = ap[j] - rc * ap[i - 1 - j];
                E = (1.0 - rc * rc) * E;
            }
            A[s][0] = 1.f;
            for (int i = 0; i < P; ++i) A[s][i + 1] = (float)(-a[i]);
        }
        float Rc[LLR_MAXP + 1];
        for (int k = 0; k <= P; ++k) Rc[k] = (float)R[0][k];
        float num = 0.f, den = 0.f;
        for (int i = 0; i <= P; ++i) {                   // row vector . toeplitz(Rc), then . column vector
            float tn = 0.f, td = 0.f;
            for (int j = 0; j <= P; ++j) {
                const float r = Rc[i > j ? i - j : j - i];
                tn += A[1][j] * r; td += A[0][j] * r;
            }
            num += tn * A[1][i]; den += td * A[0][i];
        }
        *out = logf(num / den);
    }
}

// twiddles of the n_fft-point DFT, tc / ts: f32 [n_fft]; the caller's next barrier publishes them (metric_frame_wss has one
// after it has staged the frame)
__device__ __forceinline__ void metric_wss_twiddles(float* tc, float* ts, int n_fft) {
    for (int i = threadIdx.x; i < n_fft; i += MT) {
        double s, c;
        sincos(-2.0 * 3.14159265358979323846 * (double)i / (double)n_fft, &s, &c);
        tc[i] = (float)c; ts[i] = (float)s;
    }
}

// WSS of the frame: |DFT|^2 of both windowed frames on bins 0..n_fft/2-1 (direct DFT, twiddles from LDS), 25 critical-band
// energies -> dB -> slopes -> weighted distance (sequential part on lane 0).  Thread 0 writes *out.
// fc, fp: f32 [winlength] each, sp: f32 [2][n_fft/2], red: f64 [MT], en: f64 [2][WSS_NCRIT]
__device__ __forceinline__ void metric_frame_wss(const float* __restrict__ ref, const float* __restrict__ deg, int winlength,
                                                 const double* __restrict__ window, int n_fft, const float* __restrict__ crit,
                                                 double eps, float* fc, float* fp, const float* tc, const float* ts, float* sp,
                                                 double* red, double (*en)[WSS_NCRIT], float* __restrict__ out) {
    const int half = n_fft / 2;
    for (int i = threadIdx.x; i < winlength; i += MT) {
        fc[i] = (float)((double)ref[i] * window[i]);
        fp[i] = (float)((double)deg[i] * window[i]);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < half; k += MT) {
        float cr = 0.f, ci = 0.f, pr = 0.f, pi = 0.f;
        int ph = 0;
        for (int i = 0; i < winlength; ++i) {
            const float c = tc[ph], s = ts[ph];
            cr = fmaf(fc[i], c, cr); ci = fmaf(fc[i], s, ci);
            pr = fmaf(fp[i], c, pr); pi = fmaf(fp[i], s, pi);
            ph += k; if (ph >= n_fft) ph -= n_fft;
        }
        sp[k] = cr * cr + ci * ci;
        sp[half + k] = pr * pr + pi * pi;
    }
    __syncthreads();
    for (int s = 0; s < 2; ++s)
        for (int b = 0; b < WSS_NCRIT; ++b) {
            double a = 0;
            for (int k = threadIdx.x; k < half; k += MT) a += (double)sp[s * half + k] * (double)crit[b * half + k];
            const double v = block_sum(a, red);
            if (threadIdx.x == 0) en[s][b] = 10.0 * log10(fmax(v, eps));
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int NC = WSS_NCRIT;
        double slope[2][WSS_NCRIT - 1], peak[2][WSS_NCRIT - 1], dbmax[2];
        for (int s = 0; s < 2; ++s) {
            dbmax[s] = en[s][0];
            for (int b = 1; b < NC; ++b) dbmax[s] = fmax(dbmax[s], en[s][b]);
            for (int b = 0; b < NC - 1; ++b) slope[s][b] = en[s][b + 1] - en[s][b];
            for (int i = 0; i < NC - 1; ++i) {
                int n = i;
                if (slope[s][i] > 0) {
                    while (n < NC - 1 && slope[s][n] > 0) ++n;
                    peak[s][i] = en[s][n - 1];
                } else {
                    while (n >= 0 && slope[s][n] <= 0) --n;
                    peak[s][i] = en[s][n + 1];
                }
            }
        }
        double num = 0, den = 0;
        for (int b = 0; b < NC - 1; ++b) {
            double W = 0;
            for (int s = 0; s < 2; ++s)
                W += (20.0 / (20.0 + dbmax[s] - en[s][b])) * (1.0 / (1.0 + peak[s][b] - en[s][b]));
            W *= 0.5;
            const double d = slope[0][b] - slope[1][b];
            num += W * d * d; den += W;
        }
        *out = (float)(num / den);
    }
}
