// sdr.hip -- SI-SDR and the BSS-eval SDR (Vincent et al., IEEE TASLP 14(4), 2006: bss_eval_sources with one source) of a
// ragged batch of (clean x, estimate y) clip pairs; float64 restatement: tests/sdr_reference.py.  All sums and the solve run in
// f64 (the f32 x f32 products are exact there; f32 sums cost 1e-4 .. 7e-3 dB).  One batch is a fixed launch sequence without
// host synchronisation:
//   sdr_plan_kernel     per-clip extents: info[b] = {in_off, n, chunk_off, chunks, status} (one thread, a running sum)
//  SI-SDR (oracle/frontend.py::si_sdr, optionally on mean-removed signals):
//   sdr_moments_kernel  per 4096-sample chunk: sum x, sum y (only with zero_mean); again with the means: sum x'^2, sum x'y'
//   sdr_stat_kernel     per clip, after each: the chunk sums in a fixed order -> means; alpha = <y',x'> / (<x',x'> + 1e-30)
//                       (moments of the mean-removed samples, not sum x^2 - n mean^2, which cancels under a large offset)
//   sdr_resid_kernel    per chunk, second pass with that alpha: sum (alpha x')^2, sum (alpha x' - y')^2
//   sdr_sisdr_out_kernel per clip: the chunk partials in chunk order -> out[b]
//  SDR (p = d' G^-1 d, G = toeplitz(r), r[k] = sum_t x[t] x[t+k], d[k] = sum_t x[t] y[t+k], k < L <= 512):
//   sdr_corr_kernel     per chunk: chunk + 512-sample halo in LDS (f32), each lane four consecutive lags of r and d, f64 FMAs
//   sdr_solve_kernel    per clip: partials summed in chunk order, Levinson-Durbin for a general right-hand side in LDS
// A chunk is a fixed 4096 samples from the clip's start and every reduction has a fixed shape, so a clip's bits depend on that
// clip's samples only: the same alone, in any batch and in any order.  No atomics.
#include "ragged.h"

#define SD 256
#define SD_CHUNK 4096                   // samples per chunk
#define SD_LMAX 512                     // lags the correlation kernel computes (filter_length <= 512 uses the first L)
#define SD_STAGE (SD_CHUNK + SD_LMAX)   // f32 per signal in LDS: the chunk and its halo
#define SD_INFO 5                       // int64 per clip: in_off, n, chunk_off, chunks, status
#define SD_MOM 2                        // f64 per chunk: {sum x, sum y}, then {sum x'^2, sum x'y'}
#define SD_STAT 4                       // f64 per clip: mean x, mean y, alpha, unused
#define SD_MAX_GRID 1024

__host__ __device__ static inline int64_t sdr_chunks(int64_t n) { return (n + SD_CHUNK - 1) / SD_CHUNK; }

__device__ static inline double sdr_wave_sum(double v) {                // 64 lanes, fixed order
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the same bits in every thread: lanes by butterfly, the four waves in wave order
__device__ static inline double sdr_block_sum(double v, double* red4) {
    v = sdr_wave_sum(v);
    __syncthreads();                                                     // red4 of the previous call consumed
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// A clip outside the `total` samples lengths_host summed to (ragged_clip_inside), an empty one, or one whose chunks would
// overrun the workspace sized from lengths_host gets status -1 and no work.
__global__ void sdr_plan_kernel(const int64_t* __restrict__ offsets, const int64_t* __restrict__ lengths, int nclips, int64_t total,
                                int64_t chunk_cap, int64_t* __restrict__ info) {
    if (threadIdx.x != 0) return;
    int64_t c = 0;
    for (int b = 0; b < nclips; ++b) {
        int64_t* ci = info + (int64_t)b * SD_INFO;
        const int64_t off = offsets[b], n = lengths[b];
        const bool ok = n > 0 && ragged_clip_inside(off, n, total) && c + sdr_chunks(n) <= chunk_cap;
        ci[0] = ok ? off : 0;
        ci[1] = ok ? n : 0;
        ci[2] = c;
        ci[3] = ok ? sdr_chunks(n) : 0;
        ci[4] = ok ? 0 : -1;
        if (ok) c += sdr_chunks(n);
    }
}

// per chunk, two sums: {x, y} (centered = 0) or, with the clip's means from stat, {x'^2, x'y'} (centered = 1)
__global__ __launch_bounds__(SD) void sdr_moments_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const int64_t* __restrict__ info, const double* __restrict__ stat,
                                                         int centered, double* __restrict__ mom) {
    __shared__ double red4[4];
    const int64_t* ci = info + (int64_t)blockIdx.y * SD_INFO;
    const int64_t in_off = ci[0], n = ci[1], chunk_off = ci[2], chunks = ci[3];
    const double mx = centered ? stat[(int64_t)blockIdx.y * SD_STAT] : 0.0, my = centered ? stat[(int64_t)blockIdx.y * SD_STAT + 1] : 0.0;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t t0 = c * SD_CHUNK, t1 = min(n, t0 + SD_CHUNK);
        double a0 = 0, a1 = 0;
        for (int64_t t = t0 + threadIdx.x; t < t1; t += SD) {
            const double xv = (double)x[in_off + t], yv = (double)y[in_off + t];
            if (centered) { a0 = fma(xv - mx, xv - mx, a0); a1 = fma(xv - mx, yv - my, a1); }
            else { a0 += xv; a1 += yv; }
        }
        const double s0 = sdr_block_sum(a0, red4), s1 = sdr_block_sum(a1, red4);
        if (threadIdx.x == 0) { mom[(chunk_off + c) * SD_MOM] = s0; mom[(chunk_off + c) * SD_MOM + 1] = s1; }
    }
}

// one workgroup per clip, the chunk sums in a fixed order.  which = 0: stat[b][0..1] = means of x and y (0 without
// zero_mean: mom is not read); which = 1: stat[b][2] = alpha = sum x'y' / (sum x'^2 + 1e-30)
__global__ __launch_bounds__(SD) void sdr_stat_kernel(const int64_t* __restrict__ info, const double* __restrict__ mom, int which,
                                                      int zero_mean, double* __restrict__ stat) {
    __shared__ double red4[4];
    const int64_t* ci = info + (int64_t)blockIdx.x * SD_INFO;
    const int64_t n = ci[1], chunk_off = ci[2], chunks = ci[3];
    double a0 = 0, a1 = 0;
    if (which == 1 || zero_mean)
        for (int64_t c = threadIdx.x; c < chunks; c += SD) { a0 += mom[(chunk_off + c) * SD_MOM]; a1 += mom[(chunk_off + c) * SD_MOM + 1]; }
    const double s0 = sdr_block_sum(a0, red4), s1 = sdr_block_sum(a1, red4);
    if (threadIdx.x == 0) {
        double* st = stat + (int64_t)blockIdx.x * SD_STAT;
        if (which == 0) {
            const double dn = n > 0 ? (double)n : 1.0;
            st[0] = s0 / dn; st[1] = s1 / dn; st[2] = 0.0; st[3] = 0.0;
        } else {
            st[2] = s1 / (s0 + 1e-30);
        }
    }
}

__global__ __launch_bounds__(SD) void sdr_resid_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const int64_t* __restrict__ info, const double* __restrict__ stat,
                                                       double* __restrict__ res) {
    __shared__ double red4[4];
    const int64_t* ci = info + (int64_t)blockIdx.y * SD_INFO;
    const int64_t in_off = ci[0], n = ci[1], chunk_off = ci[2], chunks = ci[3];
    const double* st = stat + (int64_t)blockIdx.y * SD_STAT;
    const double mx = st[0], my = st[1], alpha = st[2];
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t t0 = c * SD_CHUNK, t1 = min(n, t0 + SD_CHUNK);
        double at = 0, ar = 0;
        for (int64_t t = t0 + threadIdx.x; t < t1; t += SD) {
            const double tv = alpha * ((double)x[in_off + t] - mx);
            const double rv = tv - ((double)y[in_off + t] - my);
            at = fma(tv, tv, at); ar = fma(rv, rv, ar);
        }
        const double st_ = sdr_block_sum(at, red4), sr_ = sdr_block_sum(ar, red4);
        if (threadIdx.x == 0) { res[(chunk_off + c) * 2] = st_; res[(chunk_off + c) * 2 + 1] = sr_; }
    }
}

// one workgroup per clip: out[b] = {sum (alpha x')^2, sum (alpha x' - y')^2, alpha, samples (-1: not scored)}
__global__ __launch_bounds__(SD) void sdr_sisdr_out_kernel(const int64_t* __restrict__ info, const double* __restrict__ stat,
                                                           const double* __restrict__ res, double* __restrict__ out) {
    __shared__ double red4[4];
    const int64_t* ci = info + (int64_t)blockIdx.x * SD_INFO;
    const int64_t n = ci[1], chunk_off = ci[2], chunks = ci[3], status = ci[4];
    double at = 0, ar = 0;
    for (int64_t c = threadIdx.x; c < chunks; c += SD) { at += res[(chunk_off + c) * 2]; ar += res[(chunk_off + c) * 2 + 1]; }
    const double st_ = sdr_block_sum(at, red4), sr_ = sdr_block_sum(ar, red4);
    if (threadIdx.x == 0) {
        double* o = out + (int64_t)blockIdx.x * 4;
        o[0] = st_; o[1] = sr_; o[2] = stat[(int64_t)blockIdx.x * SD_STAT + 2]; o[3] = status < 0 ? -1.0 : (double)n;
    }
}

// One workgroup per chunk.  LDS holds x and y of [t0, t0 + 4096 + 512) as f32, zero past the clip's end.  Lane g of a
// 128-lane half owns lags 4g .. 4g+3 of r and d; the two halves split the chunk's samples.  Per four samples t a lane reads
// x[t .. t+3] (one address for the wave: a broadcast) and x, y [t + 4g + 4 .. + 7] (16 B per lane, consecutive lanes
// consecutive slots), keeps the eight-sample window in registers and issues 32 f64 FMAs.  part[chunk] = {r[512], d[512],
// then in ysq[chunk]: sum y^2 of the chunk}.
__global__ __launch_bounds__(SD) void sdr_corr_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                      const int64_t* __restrict__ info, double* __restrict__ part,
                                                      double* __restrict__ ysq) {
    __shared__ __attribute__((aligned(16))) float xs[SD_STAGE];
    __shared__ __attribute__((aligned(16))) float ys[SD_STAGE];
    __shared__ double comb[SD / 2][9];                                   // the second half's accumulators (padded rows)
    __shared__ double red4[4];
    const int64_t* ci = info + (int64_t)blockIdx.y * SD_INFO;
    const int64_t in_off = ci[0], n = ci[1], chunk_off = ci[2], chunks = ci[3];
    const int g = threadIdx.x & 127, half = threadIdx.x >> 7, k0 = 4 * g;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t t0 = c * SD_CHUNK;
        __syncthreads();                                                 // previous chunk's LDS consumed
        double e = 0;
        for (int i = threadIdx.x; i < SD_STAGE; i += SD) {
            const bool in = t0 + i < n;
            const float xv = in ? x[in_off + t0 + i] : 0.0f, yv = in ? y[in_off + t0 + i] : 0.0f;
            xs[i] = xv; ys[i] = yv;
            if (i < SD_CHUNK) e = fma((double)yv, (double)yv, e);
        }
        e = sdr_block_sum(e, red4);                                      // (its barriers also publish xs / ys)
        if (threadIdx.x == 0) ysq[chunk_off + c] = e;
        // samples of this chunk, rounded up to the 8 the two halves step by (the padding is zero)
        const int valid = (int)min((int64_t)SD_CHUNK, n - t0);
        const int per_half = ((valid + 7) / 8) * 4;
        double r[4] = {0, 0, 0, 0}, d[4] = {0, 0, 0, 0};
        double wx[8], wy[8];
        const int tb = half * per_half;
        {
            const float4 vx = *(const float4*)&xs[tb + k0], vy = *(const float4*)&ys[tb + k0];
            wx[0] = vx.x; wx[1] = vx.y; wx[2] = vx.z; wx[3] = vx.w;
            wy[0] = vy.x; wy[1] = vy.y; wy[2] = vy.z; wy[3] = vy.w;
        }
        for (int t = tb; t < tb + per_half; t += 4) {
            const float4 xb = *(const float4*)&xs[t];
            const float4 vx = *(const float4*)&xs[t + k0 + 4], vy = *(const float4*)&ys[t + k0 + 4];
            wx[4] = vx.x; wx[5] = vx.y; wx[6] = vx.z; wx[7] = vx.w;
            wy[4] = vy.x; wy[5] = vy.y; wy[6] = vy.z; wy[7] = vy.w;
            const double xv[4] = {xb.x, xb.y, xb.z, xb.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    r[i] = fma(xv[j], wx[j + i], r[i]);
                    d[i] = fma(xv[j], wy[j + i], d[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) { wx[i] = wx[i + 4]; wy[i] = wy[i + 4]; }
        }
        if (half == 1) {
            for (int i = 0; i < 4; ++i) { comb[g][i] = r[i]; comb[g][4 + i] = d[i]; }
        }
        __syncthreads();
        if (half == 0) {
            double* pr = part + (chunk_off + c) * (2 * SD_LMAX);
            for (int i = 0; i < 4; ++i) {
                pr[k0 + i] = r[i] + comb[g][i];
                pr[SD_LMAX + k0 + i] = d[i] + comb[g][4 + i];
            }
        }
    }
}

// One workgroup per clip.  r, d: the chunk partials in chunk order.  Then toeplitz(r[0..L)) c = d by Levinson-Durbin:
//   order m predictor a (a[m] = k):  k = -(r[m] + sum_{i=1}^{m-1} a[i] r[m-i]) / E,  a[i] += k a[m-i],  E *= 1 - k^2
//   solution:                        q = (d[m] - sum_{i=0}^{m-1} c[i] r[m-i]) / E,   c[i] += q a[m-i],  c[m] = q
// thread t holds elements t and t + 256; both dot products of a step go through one fixed-shape reduction.
// out[b] = {p = d.c, e = sum y^2, r[0], status, samples}: status 0, -1 (not scored: lengths disagree), -2 (r[0] <= 0: an
// all-zero clean clip), -3 (the prediction error stopped being positive at some order: toeplitz(r) is numerically singular).
__global__ __launch_bounds__(SD) void sdr_solve_kernel(const int64_t* __restrict__ info, const double* __restrict__ part,
                                                       const double* __restrict__ ysq, int L, double* __restrict__ out) {
    __shared__ double rr[SD_LMAX], dd[SD_LMAX], aa[SD_LMAX], cc[SD_LMAX];
    __shared__ double red4[4], red4b[4];
    const int64_t* ci = info + (int64_t)blockIdx.x * SD_INFO;
    const int64_t n = ci[1], chunk_off = ci[2], chunks = ci[3], status = ci[4];
    const int t = threadIdx.x;
    for (int k = t; k < SD_LMAX; k += SD) {
        double sr = 0, sd = 0;
        for (int64_t c = 0; c < chunks; ++c) {
            const double* pr = part + (chunk_off + c) * (2 * SD_LMAX);
            sr += pr[k]; sd += pr[SD_LMAX + k];
        }
        rr[k] = sr; dd[k] = sd; aa[k] = 0.0; cc[k] = 0.0;
    }
    double ea = 0;
    for (int64_t c = t; c < chunks; c += SD) ea += ysq[chunk_off + c];
    const double e = sdr_block_sum(ea, red4);                            // (publishes rr / dd as well)
    double st = status < 0 ? -1.0 : 0.0;
    double E = rr[0];
    if (st == 0.0 && !(E > 0.0)) st = -2.0;
    if (st == 0.0) {
        if (t == 0) cc[0] = dd[0] / E;
        __syncthreads();
        for (int m = 1; m < L; ++m) {                                    // st and E are the same bits in every thread
            double sk = 0, sq = 0;
            for (int i = t; i < m; i += SD) {
                const double rv = rr[m - i];
                sk = fma(aa[i], rv, sk);                                 // aa[0] = 0
                sq = fma(cc[i], rv, sq);
            }
            sk = sdr_wave_sum(sk); sq = sdr_wave_sum(sq);
            if ((t & 63) == 0) { red4[t >> 6] = sk; red4b[t >> 6] = sq; }
            __syncthreads();
            sk = ((red4[0] + red4[1]) + red4[2]) + red4[3];
            sq = ((red4b[0] + red4b[1]) + red4b[2]) + red4b[3];
            const double k = -(rr[m] + sk) / E;
            E = E * (1.0 - k * k);
            if (!(E > 0.0)) { st = -3.0; break; }
            const double q = (dd[m] - sq) / E;
            // new a[i] = a[i] + k a[m-i] (1 <= i < m), a[m] = k; new c[i] = c[i] + q new_a[m-i] (i < m), c[m] = q
            double an[2], ar[2];
            for (int j = 0; j < 2; ++j) {
                const int i = t + j * SD;
                an[j] = i >= 1 && i < m ? aa[i] : 0.0;
                ar[j] = i >= 1 && i < m ? aa[m - i] : 0.0;
            }
            __syncthreads();                                             // every read of the old a (and of red4) done
            for (int j = 0; j < 2; ++j) {
                const int i = t + j * SD;
                if (i >= 1 && i < m) aa[i] = fma(k, ar[j], an[j]);
                if (i == m) aa[i] = k;
            }
            __syncthreads();
            for (int j = 0; j < 2; ++j) {
                const int i = t + j * SD;
                if (i < m) cc[i] = fma(q, aa[m - i], cc[i]);
                if (i == m) cc[i] = q;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    double pa = 0;
    if (st == 0.0)
        for (int i = t; i < L; i += SD) pa = fma(dd[i], cc[i], pa);
    const double p = sdr_block_sum(pa, red4);
    if (t == 0) {
        double* o = out + (int64_t)blockIdx.x * 5;
        o[0] = p; o[1] = e; o[2] = rr[0]; o[3] = st; o[4] = status < 0 ? -1.0 : (double)n;
    }
}

namespace {
struct SdrLayout {
    int64_t total = 0, chunks = 0, max_chunks = 0;
    size_t info = 0, mom = 0, stat = 0, res = 0, part = 0, ysq = 0, bytes = 0;
};
// filter_length 0: the SI-SDR sequence's arrays; 1 .. 512: the SDR sequence's
SdrLayout sdr_layout(const int64_t* lengths, int nclips, int filter_length) {
    SdrLayout l;
    for (int b = 0; b < nclips; ++b) {
        const int64_t n = lengths[b] > 0 ? lengths[b] : 0;
        l.total += n;
        l.chunks += sdr_chunks(n);
        l.max_chunks = std::max(l.max_chunks, sdr_chunks(n));
    }
    RaggedBump ws;
    l.info = ws.take((size_t)nclips * SD_INFO * 8);
    if (filter_length == 0) {
        l.mom = ws.take((size_t)l.chunks * SD_MOM * 8);
        l.stat = ws.take((size_t)nclips * SD_STAT * 8);
        l.res = ws.take((size_t)l.chunks * 2 * 8);
    } else {
        l.part = ws.take((size_t)l.chunks * 2 * SD_LMAX * 8);
        l.ysq = ws.take((size_t)l.chunks * 8);
    }
    l.bytes = ws.o;
    return l;
}
unsigned sdr_grid_x(int64_t chunks) { return ragged_grid(chunks, 1, SD_MAX_GRID); }
}  // namespace

extern "C" int64_t sos_sdr_workspace_bytes(const int64_t* lengths_host, int nclips, int filter_length) {
    if (!ragged_clips_ok(lengths_host, nclips) || filter_length < 0 || filter_length > SD_LMAX) {
        sos_set_error("sos_sdr_workspace_bytes: bad args (1 .. 65535 clips, filter_length 0 .. %d)", SD_LMAX);
        return -1;
    }
    return (int64_t)sdr_layout(lengths_host, nclips, filter_length).bytes;
}

extern "C" int sos_sisdr_batch(const float* x, const float* y, const int64_t* offsets, const int64_t* lengths,
                               const int64_t* lengths_host, int nclips, int zero_mean, void* workspace, int64_t workspace_bytes,
                               double* out, sos_stream_t stream) {
    if (!x || !y || !offsets || !lengths || !workspace || !out) { sos_set_error("sos_sisdr_batch: null pointer"); return SOS_EINVAL; }
    if (!ragged_clips_ok(lengths_host, nclips) || (zero_mean != 0 && zero_mean != 1)) {
        sos_set_error("sos_sisdr_batch: bad args (1 .. 65535 clips, zero_mean 0 or 1)");
        return SOS_EINVAL;
    }
    const SdrLayout l = sdr_layout(lengths_host, nclips, 0);
    if (workspace_bytes < (int64_t)l.bytes) {
        sos_set_error("sos_sisdr_batch: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)l.bytes);
        return SOS_ENOSPC;
    }
    char* ws = (char*)workspace;
    int64_t* info = (int64_t*)(ws + l.info);
    double* mom = (double*)(ws + l.mom);
    double* stat = (double*)(ws + l.stat);
    double* res = (double*)(ws + l.res);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(sdr_grid_x(l.max_chunks), nclips);
    int rc;
    hipLaunchKernelGGL(sdr_plan_kernel, dim3(1), dim3(64), 0, s, offsets, lengths, nclips, l.total, l.chunks, info);
    if ((rc = sos_check_launch("sos_sisdr_batch: plan")) != SOS_OK) return rc;
    if (zero_mean) {
        hipLaunchKernelGGL(sdr_moments_kernel, grid, dim3(SD), 0, s, x, y, info, stat, 0, mom);
        if ((rc = sos_check_launch("sos_sisdr_batch: sums")) != SOS_OK) return rc;
    }
    hipLaunchKernelGGL(sdr_stat_kernel, dim3(nclips), dim3(SD), 0, s, info, mom, 0, zero_mean, stat);
    if ((rc = sos_check_launch("sos_sisdr_batch: means")) != SOS_OK) return rc;
    hipLaunchKernelGGL(sdr_moments_kernel, grid, dim3(SD), 0, s, x, y, info, stat, 1, mom);
    if ((rc = sos_check_launch("sos_sisdr_batch: moments")) != SOS_OK) return rc;
    hipLaunchKernelGGL(sdr_stat_kernel, dim3(nclips), dim3(SD), 0, s, info, mom, 1, zero_mean, stat);
    if ((rc = sos_check_launch("sos_sisdr_batch: alpha")) != SOS_OK) return rc;
    hipLaunchKernelGGL(sdr_resid_kernel, grid, dim3(SD), 0, s, x, y, info, stat, res);
    if ((rc = sos_check_launch("sos_sisdr_batch: residual")) != SOS_OK) return rc;
    hipLaunchKernelGGL(sdr_sisdr_out_kernel, dim3(nclips), dim3(SD), 0, s, info, stat, res, out);
    return sos_check_launch("sos_sisdr_batch: out");
}

extern "C" int sos_sdr_batch(const float* x, const float* y, const int64_t* offsets, const int64_t* lengths,
                             const int64_t* lengths_host, int nclips, int filter_length, int stages, void* workspace,
                             int64_t workspace_bytes, double* out, sos_stream_t stream) {
    if (!x || !y || !offsets || !lengths || !workspace || !out) { sos_set_error("sos_sdr_batch: null pointer"); return SOS_EINVAL; }
    if (!ragged_clips_ok(lengths_host, nclips) || filter_length < 1 || filter_length > SD_LMAX || stages < 1 || stages > 3) {
        sos_set_error("sos_sdr_batch: bad args (1 .. 65535 clips, filter_length 1 .. %d, got %d; stages 1 .. 3)", SD_LMAX,
                      filter_length);
        return SOS_EINVAL;
    }
    const SdrLayout l = sdr_layout(lengths_host, nclips, filter_length);
    if (workspace_bytes < (int64_t)l.bytes) {
        sos_set_error("sos_sdr_batch: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)l.bytes);
        return SOS_ENOSPC;
    }
    char* ws = (char*)workspace;
    int64_t* info = (int64_t*)(ws + l.info);
    double* part = (double*)(ws + l.part);
    double* ysq = (double*)(ws + l.ysq);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    // the plan runs for either stage, so the solve never indexes by anything but this call's own, bounds-checked extents
    hipLaunchKernelGGL(sdr_plan_kernel, dim3(1), dim3(64), 0, s, offsets, lengths, nclips, l.total, l.chunks, info);
    if ((rc = sos_check_launch("sos_sdr_batch: plan")) != SOS_OK) return rc;
    if (stages & SOS_SDR_CORRELATE) {
        hipLaunchKernelGGL(sdr_corr_kernel, dim3(sdr_grid_x(l.max_chunks), nclips), dim3(SD), 0, s, x, y, info, part, ysq);
        if ((rc = sos_check_launch("sos_sdr_batch: correlations")) != SOS_OK) return rc;
    }
    if (stages & SOS_SDR_SOLVE) {
        hipLaunchKernelGGL(sdr_solve_kernel, dim3(nclips), dim3(SD), 0, s, info, part, ysq, filter_length, out);
        if ((rc = sos_check_launch("sos_sdr_batch: solve")) != SOS_OK) return rc;
    }
    return SOS_OK;
}
