// stoi.hip -- STOI (Taal et al., IEEE TASLP 19(7), 2011) and extended STOI (Jensen & Taal, IEEE/ACM TASLP 24(11), 2016)
// of a ragged batch of (clean, processed) clip pairs, with pystoi's stoi(x, y, fs_sig, extended) contract
// (float64 restatement: tests/stoi_reference.py).  One batch is a fixed launch sequence, no host synchronisation:
//   stoi_plan_kernel      per-clip extents of every workspace array (one thread, a running sum over the clips)
//   stoi_resample_kernel  polyphase FIR to 10 kHz of x and y (Octave's resample filter, designed by the host, taps in LDS)
//   stoi_energy_kernel    20 log10(||w x_frame|| + EPS) of every 256-sample frame at hop 128 (one wave per frame, f64)
//   stoi_frames_kernel    per clip: maximum energy, keep mask (max - 40 - e < 0), ordered compaction of the kept frames
//   stoi_tob_kernel       per STFT frame of the overlap-added kept frames: f64 DFT bins 7..218, 15 third-octave bands
//   stoi_corr_kernel      per 30-frame segment: classic (clipped, per band) or extended (row+column normalised) correlation
//   stoi_sum_kernel       per clip: one fixed-order f64 sum over its segments -> out[b] = {sum, segments, kept_frames}
// Every value a clip gets depends on that clip's samples only (no atomics, no cross-clip reductions), so a clip scores the
// same bits alone, in any batch and in any order.
#include "ragged.h"

#define ST MT                           // 256 threads: the block reductions of ragged.h
#define ST_FRAME 256
#define ST_HOP 128
#define ST_NFFT 512
#define ST_NBAND 15
#define ST_NSEG 30
#define ST_BIN0 7
#define ST_NBIN 212                     // bins 7..218
#define ST_TAP_CHUNK 4096               // f64 taps per LDS pass (32 KiB)
#define ST_INFO 8                       // int64 per clip: in_off, n, sig_off, n10, f_off, F, K, status
#define ST_MAX_GRID 1024

static const double ST_EPS = 2.220446049250313e-16;    // np.finfo(float).eps
// third-octave band k covers bins [ST_EDGE[k], ST_EDGE[k+1]) (pystoi's thirdoct(10000, 512, 15, 150))
__constant__ int ST_EDGE[ST_NBAND + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

__host__ __device__ static inline int64_t stoi_n10(int64_t n, int p, int q) { return p == q ? n : (n * p + q - 1) / q; }
__host__ __device__ static inline int64_t stoi_nframes(int64_t n10) {       // starts 0, 128, ... < n10 - 256
    return n10 > ST_FRAME ? (n10 - ST_FRAME + ST_HOP - 1) / ST_HOP : 0;
}
__device__ static inline int64_t floor_div_d(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// np.hanning(258)[1:-1]
__device__ static inline double stoi_window(int s) { return 0.5 - 0.5 * cos(2.0 * M_PI * (double)(s + 1) / 257.0); }

__device__ static inline double half_wave_sum(double v) {           // over the 32 lanes of a half wave, fixed order
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
    return v;
}

// info[b] = {in_off, n, sig_off, n10, f_off, F, K = 0, status}: the signal the frames read starts at sig_off (the input
// itself at 10 kHz, else the resampled copy), frame-indexed arrays at f_off.  A clip outside the s_cap samples the host
// summed (ragged_clip_inside), or whose extent would overrun the workspace sized from the host's lengths, gets status -1 and
// no work.
__global__ void stoi_plan_kernel(const int64_t* __restrict__ offsets, const int64_t* __restrict__ lengths, int nclips, int p, int q,
                                 int64_t s_cap, int64_t r_cap, int64_t f_cap, int64_t* __restrict__ info) {
    if (threadIdx.x != 0) return;
    int64_t r = 0, f = 0;
    for (int b = 0; b < nclips; ++b) {
        int64_t* ci = info + (int64_t)b * ST_INFO;
        const int64_t n = lengths[b] > 0 ? lengths[b] : 0, off = offsets[b];
        const int64_t n10 = stoi_n10(n, p, q), F = stoi_nframes(n10);
        const bool ok = ragged_clip_inside(off, n, s_cap) && (p == q || r + n10 <= r_cap) && f + F <= f_cap;
        ci[0] = ok ? off : 0;
        ci[1] = ok ? n : 0;
        ci[2] = p == q ? ci[0] : r;
        ci[3] = ok ? n10 : 0;
        ci[4] = f;
        ci[5] = ok ? F : 0;
        ci[6] = 0;
        ci[7] = ok ? 0 : -1;
        if (ok) { r += p == q ? 0 : n10; f += F; }
    }
}

// y[m] = sum_i x[i] h[L + m q - i p] over the taps inside h (h already scaled by p): scipy.signal.resample_poly's
// zero-phase alignment, ceil(n p / q) outputs.  Long filters (low common rates such as 44.1 kHz) pass through LDS in chunks.
__global__ __launch_bounds__(ST) void stoi_resample_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const int64_t* __restrict__ info, int p, int q,
                                                           const double* __restrict__ taps, int ntaps, float* __restrict__ rx,
                                                           float* __restrict__ ry) {
    __shared__ double h[ST_TAP_CHUNK];
    const int64_t* ci = info + (int64_t)blockIdx.y * ST_INFO;
    const int64_t in_off = ci[0], n = ci[1], out_off = ci[2], n10 = ci[3];
    const int L = (ntaps - 1) / 2;
    const bool one = ntaps <= ST_TAP_CHUNK;
    if (one) {
        for (int i = threadIdx.x; i < ntaps; i += ST) h[i] = taps[i];
        __syncthreads();
    }
    const float* xs = x + in_off;
    const float* ys = y + in_off;
    for (int64_t c0 = (int64_t)blockIdx.x * ST; c0 < n10; c0 += (int64_t)gridDim.x * ST) {
        const int64_t m = c0 + threadIdx.x;
        const int64_t c = (int64_t)L + m * q;
        double ax = 0, ay = 0;
        for (int t0 = 0; t0 < ntaps; t0 += ST_TAP_CHUNK) {
            const int t1 = min(ntaps, t0 + ST_TAP_CHUNK);
            if (!one) {
                __syncthreads();
                for (int i = t0 + threadIdx.x; i < t1; i += ST) h[i - t0] = taps[i];
                __syncthreads();
            }
            if (m < n10) {
                // tap index c - i p inside [t0, t1)
                const int64_t ilo = max(floor_div_d(c - t1, p) + 1, (int64_t)0);
                const int64_t ihi = min(floor_div_d(c - t0, p), n - 1);
                for (int64_t i = ilo; i <= ihi; ++i) {
                    const double w = h[c - i * p - t0];
                    ax = fma(w, (double)xs[i], ax);
                    ay = fma(w, (double)ys[i], ay);
                }
            }
        }
        if (m < n10) { rx[out_off + m] = (float)ax; ry[out_off + m] = (float)ay; }
    }
}

// one wave per frame: energy[f_off + f] = 20 log10(sqrt(sum (w x)^2) + EPS)
__global__ __launch_bounds__(ST) void stoi_energy_kernel(const float* __restrict__ sx, const int64_t* __restrict__ info,
                                                         double* __restrict__ energy) {
    const int64_t* ci = info + (int64_t)blockIdx.y * ST_INFO;
    const int64_t sig_off = ci[2], f_off = ci[4], F = ci[5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double w[4];
    for (int k = 0; k < 4; ++k) w[k] = stoi_window(lane + 64 * k);
    for (int64_t f = (int64_t)blockIdx.x * 4 + wave; f < F; f += (int64_t)gridDim.x * 4) {
        const float* fr = sx + sig_off + f * ST_HOP;
        double a = 0;
        for (int k = 0; k < 4; ++k) {
            const double v = w[k] * (double)fr[lane + 64 * k];
            a = fma(v, v, a);
        }
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) energy[f_off + f] = 20.0 * log10(sqrt(a) + ST_EPS);
    }
}

// one workgroup per clip: frames with max_energy - 40 - energy < 0 stay; their indices, in order, go to kept[f_off ..],
// their count to info[b][6] (chunked prefix scan, as metric_compact_kernel: any clip length)
__global__ __launch_bounds__(ST) void stoi_frames_kernel(const double* __restrict__ energy, int64_t* __restrict__ info,
                                                         int* __restrict__ kept) {
    __shared__ double red[ST];
    __shared__ int scan[ST];
    __shared__ int64_t base;
    int64_t* ci = info + (int64_t)blockIdx.x * ST_INFO;
    const int64_t f_off = ci[4], F = ci[5];
    double mx = -INFINITY;
    for (int64_t f = threadIdx.x; f < F; f += ST) mx = fmax(mx, energy[f_off + f]);
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = ST / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const double emax = red[0];
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < F; c0 += ST) {
        const int64_t f = c0 + threadIdx.x;
        const int keep = (f < F && emax - 40.0 - energy[f_off + f] < 0.0) ? 1 : 0;
        scan[threadIdx.x] = keep;
        __syncthreads();
        for (int s = 1; s < ST; s <<= 1) {
            const int v = (int)threadIdx.x >= s ? scan[threadIdx.x - s] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        if (keep) kept[f_off + base + scan[threadIdx.x] - 1] = (int)f;
        __syncthreads();
        if (threadIdx.x == 0) base += scan[ST - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) ci[6] = base;
}

// one workgroup per STFT frame j < K-1 of the overlap-added kept frames: sample s of frame j is w[s] x[kept j][s] plus
// w[s+128] x[kept j-1][s+128] (s < 128, j > 0) or w[s-128] x[kept j+1][s-128] (s >= 128); it is windowed again,
// zero-padded to 512 and transformed on bins 7..218 (f64); tob[f_off + j] = {sqrt(band power of x) [15], of y [15]}
__global__ __launch_bounds__(ST) void stoi_tob_kernel(const float* __restrict__ sx, const float* __restrict__ sy,
                                                      const int64_t* __restrict__ info, const int* __restrict__ kept,
                                                      double* __restrict__ tob) {
    __shared__ double tw_c[ST_NFFT], tw_s[ST_NFFT];
    __shared__ double fx[ST_FRAME], fy[ST_FRAME];
    __shared__ double px[ST_NBIN], py[ST_NBIN];
    const int64_t* ci = info + (int64_t)blockIdx.y * ST_INFO;
    const int64_t sig_off = ci[2], f_off = ci[4], K = ci[6];
    const int t = threadIdx.x;
    for (int i = t; i < ST_NFFT; i += ST) {
        double s, c;
        sincospi(-2.0 * (double)i / (double)ST_NFFT, &s, &c);
        tw_c[i] = c; tw_s[i] = s;
    }
    const double w0 = stoi_window(t);
    const double wn = stoi_window(t < ST_HOP ? t + ST_HOP : t - ST_HOP);
    for (int64_t j = blockIdx.x; j < K - 1; j += gridDim.x) {
        __syncthreads();                                 // twiddles written / previous frame's LDS consumed
        const int64_t s0 = sig_off + (int64_t)kept[f_off + j] * ST_HOP + t;
        double vx = w0 * (double)sx[s0], vy = w0 * (double)sy[s0];
        const int64_t jn = t < ST_HOP ? j - 1 : j + 1;  // the neighbour kept frame overlapping this half
        if (jn >= 0) {
            const int64_t s1 = sig_off + (int64_t)kept[f_off + jn] * ST_HOP + (t < ST_HOP ? t + ST_HOP : t - ST_HOP);
            vx = fma(wn, (double)sx[s1], vx);
            vy = fma(wn, (double)sy[s1], vy);
        }
        fx[t] = w0 * vx; fy[t] = w0 * vy;
        __syncthreads();
        if (t < ST_NBIN) {
            const int k = ST_BIN0 + t;
            double xr = 0, xi = 0, yr = 0, yi = 0;
            int ph = 0;
            for (int s = 0; s < ST_FRAME; ++s) {
                const double c = tw_c[ph], sn = tw_s[ph];
                xr = fma(fx[s], c, xr); xi = fma(fx[s], sn, xi);
                yr = fma(fy[s], c, yr); yi = fma(fy[s], sn, yi);
                ph = (ph + k) & (ST_NFFT - 1);
            }
            px[t] = xr * xr + xi * xi;
            py[t] = yr * yr + yi * yi;
        }
        __syncthreads();
        if (t < 2 * ST_NBAND) {
            const int b = t % ST_NBAND;
            const double* pw = t < ST_NBAND ? px : py;
            double a = 0;
            for (int k = ST_EDGE[b]; k < ST_EDGE[b + 1]; ++k) a += pw[k - ST_BIN0];
            tob[(f_off + j) * (2 * ST_NBAND) + t] = sqrt(a);
        }
    }
}

// one half wave per 30-frame segment (frames s .. s+29 of the clip's STFT frames), lane n < 30 holding frame s+n's 15 band
// values of x and y; segv[f_off + s] = sum over bands of the classic correlation, or sum_n x_n . y_n / 30 (extended)
__global__ __launch_bounds__(ST) void stoi_corr_kernel(const int64_t* __restrict__ info, const double* __restrict__ tob,
                                                       int extended, double* __restrict__ segv) {
    const int64_t* ci = info + (int64_t)blockIdx.y * ST_INFO;
    const int64_t f_off = ci[4], K = ci[6];
    const int64_t S = K - 1 - (ST_NSEG - 1);              // segments: STFT frames K-1, windows of 30
    const int lane = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1, wave = threadIdx.x >> 6;
    const bool act = lane < ST_NSEG;
    const double clip = 1.0 + pow(10.0, 15.0 / 20.0);     // 1 + 10^(-BETA/20), BETA = -15
    for (int64_t s0 = ((int64_t)blockIdx.x * 4 + wave) * 2; s0 < S; s0 += (int64_t)gridDim.x * 8) {
        const int64_t s = s0 + half;
        const bool valid = s < S;
        double xb[ST_NBAND], yb[ST_NBAND];
        const double* tp = tob + (f_off + s + lane) * (2 * ST_NBAND);
        for (int b = 0; b < ST_NBAND; ++b) {
            xb[b] = (valid && act) ? tp[b] : 0.0;
            yb[b] = (valid && act) ? tp[ST_NBAND + b] : 0.0;
        }
        double d = 0;
        if (!extended) {
            for (int b = 0; b < ST_NBAND; ++b) {
                const double nx = sqrt(half_wave_sum(xb[b] * xb[b])), ny = sqrt(half_wave_sum(yb[b] * yb[b]));
                const double yp = fmin(yb[b] * (nx / (ny + ST_EPS)), xb[b] * clip);
                const double mx = half_wave_sum(xb[b]) / ST_NSEG, my = half_wave_sum(yp) / ST_NSEG;
                const double xc = act ? xb[b] - mx : 0.0, yc = act ? yp - my : 0.0;
                const double nxc = sqrt(half_wave_sum(xc * xc)), nyc = sqrt(half_wave_sum(yc * yc));
                d += half_wave_sum((xc / (nxc + ST_EPS)) * (yc / (nyc + ST_EPS)));
            }
        } else {
            for (int b = 0; b < ST_NBAND; ++b) {                  // rows: each band over the 30 frames
                const double mx = half_wave_sum(xb[b]) / ST_NSEG, my = half_wave_sum(yb[b]) / ST_NSEG;
                const double xc = act ? xb[b] - mx : 0.0, yc = act ? yb[b] - my : 0.0;
                const double nxc = sqrt(half_wave_sum(xc * xc)), nyc = sqrt(half_wave_sum(yc * yc));
                xb[b] = xc / (nxc + ST_EPS);
                yb[b] = yc / (nyc + ST_EPS);
            }
            double mx = 0, my = 0;                                 // columns: each frame over the 15 bands (in-lane)
            for (int b = 0; b < ST_NBAND; ++b) { mx += xb[b]; my += yb[b]; }
            mx /= ST_NBAND; my /= ST_NBAND;
            double nx = 0, ny = 0;
            for (int b = 0; b < ST_NBAND; ++b) {
                xb[b] -= mx; yb[b] -= my;
                nx = fma(xb[b], xb[b], nx); ny = fma(yb[b], yb[b], ny);
            }
            nx = sqrt(nx) + ST_EPS; ny = sqrt(ny) + ST_EPS;
            double dot = 0;
            for (int b = 0; b < ST_NBAND; ++b) dot = fma(xb[b] / nx, yb[b] / ny, dot);
            d = half_wave_sum(act ? dot : 0.0) / ST_NSEG;
        }
        if (valid && lane == 0) segv[f_off + s] = d;
    }
}

// one workgroup per clip: out[b] = {sum of the segment values (fixed order), segments, kept frames (-1: not scored)}
__global__ __launch_bounds__(ST) void stoi_sum_kernel(const int64_t* __restrict__ info, const double* __restrict__ segv,
                                                      double* __restrict__ out) {
    __shared__ double red[ST];
    const int64_t* ci = info + (int64_t)blockIdx.x * ST_INFO;
    const int64_t f_off = ci[4], K = ci[6];
    const int64_t S = K - 1 - (ST_NSEG - 1) > 0 ? K - 1 - (ST_NSEG - 1) : 0;
    double a = 0;
    for (int64_t s = threadIdx.x; s < S; s += ST) a += segv[f_off + s];
    const double tot = block_sum(a, red);
    if (threadIdx.x == 0) {
        out[3 * blockIdx.x] = tot;
        out[3 * blockIdx.x + 1] = (double)S;
        out[3 * blockIdx.x + 2] = ci[7] < 0 ? -1.0 : (double)K;
    }
}

namespace {
struct StoiLayout {
    int64_t s_total = 0, r_total = 0, f_total = 0, max_n10 = 0, max_f = 0;
    size_t info = 0, rx = 0, ry = 0, energy = 0, kept = 0, tob = 0, segv = 0, bytes = 0;
};
StoiLayout stoi_layout(const int64_t* lengths, int nclips, int p, int q) {
    StoiLayout l;
    for (int b = 0; b < nclips; ++b) {
        const int64_t n = lengths[b] > 0 ? lengths[b] : 0, n10 = stoi_n10(n, p, q), F = stoi_nframes(n10);
        l.s_total += n;
        l.r_total += p == q ? 0 : n10;
        l.f_total += F;
        l.max_n10 = std::max(l.max_n10, n10);
        l.max_f = std::max(l.max_f, F);
    }
    RaggedBump ws;
    l.info = ws.take((size_t)nclips * ST_INFO * 8);
    l.rx = ws.take((size_t)l.r_total * 4);
    l.ry = ws.take((size_t)l.r_total * 4);
    l.energy = ws.take((size_t)l.f_total * 8);
    l.kept = ws.take((size_t)l.f_total * 4);
    l.tob = ws.take((size_t)l.f_total * 2 * ST_NBAND * 8);
    l.segv = ws.take((size_t)l.f_total * 8);
    l.bytes = ws.o;
    return l;
}
unsigned grid_x(int64_t units, int per_block) { return ragged_grid(units, per_block, ST_MAX_GRID); }
bool stoi_args_ok(const int64_t* lengths, int nclips, int p, int q) {
    return ragged_clips_ok(lengths, nclips) && p > 0 && q > 0 && (int64_t)p * q <= (1 << 30);
}
}  // namespace

extern "C" int64_t sos_stoi_workspace_bytes(const int64_t* lengths, int nclips, int p, int q) {
    if (!stoi_args_ok(lengths, nclips, p, q)) { sos_set_error("sos_stoi_workspace_bytes: bad args"); return -1; }
    return (int64_t)stoi_layout(lengths, nclips, p, q).bytes;
}

extern "C" int sos_stoi_batch(const float* x, const float* y, const int64_t* offsets, const int64_t* lengths,
                              const int64_t* lengths_host, int nclips, int p, int q, const double* taps, int ntaps, int extended,
                              void* workspace, int64_t workspace_bytes, double* out, sos_stream_t stream) {
    if (!x || !y || !offsets || !lengths || !workspace || !out || !stoi_args_ok(lengths_host, nclips, p, q) ||
        (extended != 0 && extended != 1) || (p != q && (!taps || ntaps < 1 || (ntaps & 1) == 0))) {
        sos_set_error("sos_stoi_batch: bad args");
        return SOS_EINVAL;
    }
    const StoiLayout l = stoi_layout(lengths_host, nclips, p, q);
    if (workspace_bytes < (int64_t)l.bytes) {
        sos_set_error("sos_stoi_batch: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)l.bytes);
        return SOS_EINVAL;
    }
    char* ws = (char*)workspace;
    int64_t* info = (int64_t*)(ws + l.info);
    float* rx = (float*)(ws + l.rx);
    float* ry = (float*)(ws + l.ry);
    double* energy = (double*)(ws + l.energy);
    int* kept = (int*)(ws + l.kept);
    double* tob = (double*)(ws + l.tob);
    double* segv = (double*)(ws + l.segv);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    hipLaunchKernelGGL(stoi_plan_kernel, dim3(1), dim3(64), 0, s, offsets, lengths, nclips, p, q, l.s_total, l.r_total,
                       l.f_total, info);
    if ((rc = sos_check_launch("sos_stoi_batch: plan")) != SOS_OK) return rc;
    const float* sx = x;
    const float* sy = y;
    if (p != q) {
        hipLaunchKernelGGL(stoi_resample_kernel, dim3(grid_x(l.max_n10, ST), nclips), dim3(ST), 0, s, x, y, info, p, q, taps, ntaps,
                           rx, ry);
        if ((rc = sos_check_launch("sos_stoi_batch: resample")) != SOS_OK) return rc;
        sx = rx; sy = ry;
    }
    hipLaunchKernelGGL(stoi_energy_kernel, dim3(grid_x(l.max_f, 4), nclips), dim3(ST), 0, s, sx, info, energy);
    if ((rc = sos_check_launch("sos_stoi_batch: energy")) != SOS_OK) return rc;
    hipLaunchKernelGGL(stoi_frames_kernel, dim3(nclips), dim3(ST), 0, s, energy, info, kept);
    if ((rc = sos_check_launch("sos_stoi_batch: frames")) != SOS_OK) return rc;
    hipLaunchKernelGGL(stoi_tob_kernel, dim3(grid_x(l.max_f, 1), nclips), dim3(ST), 0, s, sx, sy, info, kept, tob);
    if ((rc = sos_check_launch("sos_stoi_batch: tob")) != SOS_OK) return rc;
    hipLaunchKernelGGL(stoi_corr_kernel, dim3(grid_x(l.max_f, 8), nclips), dim3(ST), 0, s, info, tob, extended, segv);
    if ((rc = sos_check_launch("sos_stoi_batch: corr")) != SOS_OK) return rc;
    hipLaunchKernelGGL(stoi_sum_kernel, dim3(nclips), dim3(ST), 0, s, info, segv, out);
    return sos_check_launch("sos_stoi_batch: sum");
}
