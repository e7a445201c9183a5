// metrics.hip -- per-sample / per-frame work of the objective measures of M2/metrics.py:
// segmental SNR family (metrics_ssnr :86-130, _shift :132-176, _exclude_silence :178-244), llr :561-623 with
// lpcoeff :626-681, wss :404-558, metrics_L1 :40-45.  The kernels reduce the signals to per-frame quantities (frame
// energies, LPC log-likelihood ratios, weighted spectral slope distances); the few-thousand-element finalisation
// (log10 / clamp / mean / trimmed mean / composite formulas) is host code in sos_amd/metrics.py.
// Frames: start = f * skip, `winlength` samples, window w[i] = 0.5 (1 - cos(2 pi (i+1) / (winlength+1))).
#include "metrics_frame.h"           // the per-frame arithmetic shared with metrics_batch.hip; MT and the block reductions

// out[0] = sum ref^2, out[1] = sum (ref - deg)^2, out[2] = max |ref|   (single workgroup: evaluation sizes)
__global__ __launch_bounds__(MT) void metric_totals_kernel(const float* __restrict__ ref, const float* __restrict__ deg,
                                                            long long n, double* __restrict__ out) {
    __shared__ double red[MT];
    double a = 0, b = 0, m = 0;
    for (long long i = threadIdx.x; i < n; i += MT) {
        const double r = ref[i], d = r - (double)deg[i];
        a += r * r; b += d * d;
        m = fmax(m, fabs(r));
    }
    const double sa = block_sum(a, red), sb = block_sum(b, red), sm = block_max(m, red);
    if (threadIdx.x == 0) { out[0] = sa; out[1] = sb; out[2] = sm; }
}

// one workgroup per frame: out[f][0] = sum (w c)^2, out[f][1] = sum (w c - w p)^2
__global__ __launch_bounds__(MT) void metric_frame_energy_kernel(const float* __restrict__ ref, const float* __restrict__ deg,
                                                                  int winlength, int skip, const double* __restrict__ window,
                                                                  double* __restrict__ out) {
    __shared__ double red[MT];
    const long long start = (long long)blockIdx.x * skip;
    double sa, sb;
    metric_frame_energy(ref + start, deg + start, winlength, window, red, sa, sb);
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = sa; out[2 * blockIdx.x + 1] = sb; }
}

// order-preserving compaction of the samples with |clean| >= thr (single workgroup, chunked prefix scan)
__global__ __launch_bounds__(MT) void metric_compact_kernel(const float* __restrict__ clean, const float* __restrict__ proc,
                                                             long long n, float thr, float* __restrict__ oc,
                                                             float* __restrict__ op, long long* __restrict__ count) {
    __shared__ int scan[MT];
    __shared__ long long base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (long long c0 = 0; c0 < n; c0 += MT) {
        const long long i = c0 + threadIdx.x;
        const int keep = (i < n && !(fabsf(clean[i]) < thr)) ? 1 : 0;
        const int incl = block_scan_incl(keep, scan);
        if (keep) { const long long o = base + incl - 1; oc[o] = clean[i]; op[o] = proc[i]; }
        __syncthreads();
        if (threadIdx.x == 0) base += scan[MT - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

// LLR of one frame per workgroup (metric_frame_llr)
__global__ __launch_bounds__(MT) void metric_llr_kernel(const float* __restrict__ ref, const float* __restrict__ deg, int winlength,
                                                         int skip, const double* __restrict__ window, int P,
                                                         float* __restrict__ out) {
    extern __shared__ double fr[];                      // [2][winlength]
    __shared__ double red[MT];
    __shared__ double R[2][LLR_MAXP + 1];
    const long long start = (long long)blockIdx.x * skip;
    metric_frame_llr(ref + start, deg + start, winlength, window, P, fr, red, R, out + blockIdx.x);
}

// WSS of one frame per workgroup (metric_frame_wss)
__global__ __launch_bounds__(MT) void metric_wss_kernel(const float* __restrict__ ref, const float* __restrict__ deg, int winlength,
                                                         int skip, const double* __restrict__ window, int n_fft,
                                                         const float* __restrict__ crit, double eps, float* __restrict__ out) {
    extern __shared__ float sm[];                       // frames [2][winlength], twiddle cos/sin [n_fft] each, spectra [2][n_fft/2]
    float* fc = sm;
    float* fp = sm + winlength;
    float* tc = fp + winlength;
    float* ts = tc + n_fft;
    float* sp = ts + n_fft;
    __shared__ double red[MT];
    __shared__ double en[2][WSS_NCRIT];
    const long long start = (long long)blockIdx.x * skip;
    metric_wss_twiddles(tc, ts, n_fft);
    metric_frame_wss(ref + start, deg + start, winlength, window, n_fft, crit, eps, fc, fp, tc, ts, sp, red, en, out + blockIdx.x);
}

// mean | lerp(output)(steps) - target |, steps = linspace(0, n_out - 1, n_t)   (scipy interp1d + np.linspace)
__global__ __launch_bounds__(MT) void metric_l1_kernel(const float* __restrict__ outp, long long n_out, const float* __restrict__ target,
                                                        long long n_t, double* __restrict__ res) {
    __shared__ double red[MT];
    double a = 0;
    const double step = n_t > 1 ? (double)(n_out - 1) / (double)(n_t - 1) : 0.0;
    for (long long j = threadIdx.x; j < n_t; j += MT) {
        double x = (double)j * step;
        if (j == n_t - 1) x = (double)(n_out - 1);
        long long i0 = (long long)x;
        if (i0 > n_out - 2) i0 = n_out - 2 > 0 ? n_out - 2 : 0;
        const double f = x - (double)i0;
        const double v = n_out > 1 ? (double)outp[i0] + f * ((double)outp[i0 + 1] - (double)outp[i0]) : (double)outp[0];
        a += fabs(v - (double)target[j]);
    }
    const double s = block_sum(a, red);
    if (threadIdx.x == 0) res[0] = s / (double)n_t;
}

#define MCHK(c, name) if (!(c)) { sos_set_error(name ": bad args"); return SOS_EINVAL; }

extern "C" int sos_metric_totals(const float* ref, const float* deg, int64_t n, double* out3, sos_stream_t stream) {
    MCHK(ref && deg && out3 && n > 0, "sos_metric_totals")
    hipLaunchKernelGGL(metric_totals_kernel, dim3(1), dim3(MT), 0, (hipStream_t)stream, ref, deg, (long long)n, out3);
    return sos_check_launch("sos_metric_totals");
}
extern "C" int sos_metric_frame_energy(const float* ref, const float* deg, int64_t n, int winlength, int skip, int64_t num_frames,
                                       const double* window, double* out, sos_stream_t stream) {
    MCHK(ref && deg && window && out && winlength > 0 && skip > 0 && num_frames > 0 && (num_frames - 1) * skip + winlength <= n,
         "sos_metric_frame_energy")
    hipLaunchKernelGGL(metric_frame_energy_kernel, dim3((unsigned)num_frames), dim3(MT), 0, (hipStream_t)stream, ref, deg, winlength,
                       skip, window, out);
    return sos_check_launch("sos_metric_frame_energy");
}
extern "C" int sos_metric_compact(const float* clean, const float* proc, int64_t n, float thr, float* out_clean, float* out_proc,
                                  int64_t* count, sos_stream_t stream) {
    MCHK(clean && proc && out_clean && out_proc && count && n > 0, "sos_metric_compact")
    hipLaunchKernelGGL(metric_compact_kernel, dim3(1), dim3(MT), 0, (hipStream_t)stream, clean, proc, (long long)n, thr, out_clean,
                       out_proc, (long long*)count);
    return sos_check_launch("sos_metric_compact");
}
extern "C" int sos_metric_llr(const float* ref, const float* deg, int64_t n, int winlength, int skip, int64_t num_frames,
                              const double* window, int P, float* out, sos_stream_t stream) {
    MCHK(ref && deg && window && out && winlength > 0 && skip > 0 && num_frames > 0 && P > 0 && P <= LLR_MAXP && P < winlength &&
         (num_frames - 1) * skip + winlength <= n && (size_t)winlength * 16 <= 64 * 1024, "sos_metric_llr")
    hipLaunchKernelGGL(metric_llr_kernel, dim3((unsigned)num_frames), dim3(MT), (size_t)winlength * 16, (hipStream_t)stream, ref, deg,
                       winlength, skip, window, P, out);
    return sos_check_launch("sos_metric_llr");
}
extern "C" int sos_metric_wss(const float* ref, const float* deg, int64_t n, int winlength, int skip, int64_t num_frames,
                              const double* window, int n_fft, const float* crit_filter, double eps, float* out, sos_stream_t stream) {
    const size_t lds = ((size_t)2 * winlength + 2 * (size_t)n_fft + (size_t)n_fft) * 4;
    MCHK(ref && deg && window && crit_filter && out && winlength > 0 && skip > 0 && num_frames > 0 && n_fft >= winlength &&
         (n_fft & (n_fft - 1)) == 0 && (num_frames - 1) * skip + winlength <= n && lds <= 60 * 1024, "sos_metric_wss")
    hipLaunchKernelGGL(metric_wss_kernel, dim3((unsigned)num_frames), dim3(MT), lds, (hipStream_t)stream, ref, deg, winlength, skip,
                       window, n_fft, crit_filter, eps, out);
    return sos_check_launch("sos_metric_wss");
}
extern "C" int sos_metric_l1(const float* output, int64_t n_out, const float* target, int64_t n_t, double* result, sos_stream_t stream) {
    MCHK(output && target && result && n_out > 0 && n_t > 0, "sos_metric_l1")
    hipLaunchKernelGGL(metric_l1_kernel, dim3(1), dim3(MT), 0, (hipStream_t)stream, output, (long long)n_out, target, (long long)n_t, result);
    return sos_check_launch("sos_metric_l1");
}
