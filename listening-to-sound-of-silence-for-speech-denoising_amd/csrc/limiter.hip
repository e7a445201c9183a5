// limiter.hip -- the look-ahead limiter between the loudness gain and the encode (audio_io.limit_batch_device; float64 / numpy
// restatement: tests/limiter_reference.py).  sos_limiter_batch_f32 brings every file of a group to its target loudness by the
// gain s AND holds its peaks at a ceiling C by a gain curve g[t] <= 1 that dips around the peaks only; one curve per file for all
// its channels.  Out of place (a tile reads a halo its neighbour would overwrite), three launches, no wait for the device.
// The rule, per file, with m = min(frames, available) and every sample outside [0, m) reading 0:
//   s     = (float) 10^((T - L) / 20) in double, 1 where L or T is not finite;  C = (float) 10^(ceiling / 20), taken on the host
//   p[t]  = max over channels of |x_c[t]|; under the true peak also of the six interpolated points next to t, t - 1 + q / 4 and
//           t + q / 4 for q = 1, 2, 3 (tp_point of loudness_core.h: the points sos_true_peak_batch_f64 forms)
//   r[t]  = a > C ? max((float)((double)C / (double)a), 2^-10) : 1 with a = s * p[t] in float32; 1 outside [0, m)
//   mn[t] = min r[t - H .. t + H];  g[t] = (float)((sum of (double)mn[t - H .. t + H]) / (2 H + 1));  y_c[t] = x_c[t] * (g[t] * s)
// Every mn is a multiple of 2^-33 in [2^-10, 1], so a float64 sum of up to 2^13 of them is exact in any order: the prefix sums
// below give the bits a sliding sum or a tree would.  t is inside the window of every mn[u] that g[t] averages, so g[t] <= r[t].
//   lim_init_kernel    rows[f] = {s, 1, 0, 0}, or {NaN, NaN, -1, 0} for a row that fails the rule
//   lim_kernel         a FLAT grid over the time tiles of all files (the file search of tp_peak_kernel): a workgroup owns
//                      LIM_TILE samples of time for ALL channels of its file.  Three float arrays of E = LIM_TILE + 4 H + 12 in LDS:
//                      every channel's tile and its halo of 2 H (+ 6) is staged in 16-byte lines wherever the plane starts and
//                      folded into p; r; the sliding minimum by doubling (floor(log2(2 H + 1)) passes between two of the arrays
//                      and one that joins two overlapping power-of-two windows); float64 prefix sums of mn over the two arrays
//                      that are free by then; g * s; the channels are read again and y stored in 16-byte lines.  A tile without
//                      a sample over the ceiling (most of them) skips from r to the store.  Samples [m, available) are copied.
//                      min g: an atomic minimum on the bits of the positive double; samples with g < 1: an integer atomic add.
//                      Neither has an order: two calls give equal bits.
//   lim_finish_kernel  the integer count of column 2 becomes the double the row is read as
// Bounds: the rule of ragged.h -- the host refuses a row of table_host outside the totals it summed or with H outside 1 .. 1024
// (SOS_EINVAL, naming the file), the kernels skip a row of the DEVICE table that fails the same rule or whose H exceeds the
// largest the host sized the LDS for.
#include "loudness_core.h"
#include <math.h>

#define LIM_THREADS 512
#define LIM_TILE SOS_LIMITER_TILE       // 4096 samples of time per workgroup; (LIM_TILE + 4 H) / LIM_TILE = 1.23 at H = 240 (5 ms at 48 kHz)
#define LIM_MAX_H 1024
#define LIM_FLOOR 0.0009765625f         // 2^-10: the least r, -60 dB
#define LIM_MAX_GRID 8192
#define LIM_LDS(hmax) ((LIM_TILE + 4 * (hmax) + 12) * 3 * (int)sizeof(float))

struct LimRow { int64_t first, avail, ch, m, H, tiles; };

__host__ __device__ static inline bool lim_row(const int64_t* te, int64_t total_in, int64_t hmax, LimRow* r) {
    *r = {te[0], te[1], te[2], 0, te[4], 0};
    const int64_t frames = te[3];
    if (!ld_planes_inside(r->first, r->avail, r->ch, total_in) || frames < 0 || r->H < 1 || r->H > hmax) return false;
    r->m = ld_min(frames, r->avail);
    r->tiles = (r->avail + LIM_TILE - 1) / LIM_TILE;
    return true;
}

__device__ __forceinline__ float lim_s(const double* stats, const double* targets, int64_t f) {
    const double L = stats[f * 4], T = targets[f];
    return isfinite(L) && isfinite(T) ? (float)pow(10.0, (T - L) / 20.0) : 1.f;
}

__global__ void lim_init_kernel(const int64_t* __restrict__ table, int nfiles, int64_t total_in, int hmax,
                                const double* __restrict__ stats, const double* __restrict__ targets, double* __restrict__ rows) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nfiles) return;
    LimRow r;
    const bool ok = lim_row(table + (int64_t)f * LD_COLS, total_in, hmax, &r);
    double* out = rows + (int64_t)f * 4;
    out[0] = ok ? (double)lim_s(stats, targets, f) : (double)NAN;
    out[1] = ok ? 1.0 : (double)NAN;
    out[2] = ok ? 0.0 : -1.0;                                        // the bits of the integer 0 until lim_finish_kernel
    out[3] = 0.0;
}

__global__ void lim_finish_kernel(const int64_t* __restrict__ table, int nfiles, int64_t total_in, int hmax, double* __restrict__ rows) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nfiles) return;
    LimRow r;
    if (!lim_row(table + (int64_t)f * LD_COLS, total_in, hmax, &r)) return;
    rows[(int64_t)f * 4 + 2] = (double)__double_as_longlong(rows[(int64_t)f * 4 + 2]);
}

template <bool TRUE_PEAK>
__global__ __launch_bounds__(LIM_THREADS) void lim_kernel(const float* __restrict__ planes, float* __restrict__ out,
                                                          const int64_t* __restrict__ table, int nfiles, int64_t total_in,
                                                          int64_t total_tiles, int hmax, const double* __restrict__ stats,
                                                          const double* __restrict__ targets, float C, const float* __restrict__ coef,
                                                          double* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [3][E]
    __shared__ int64_t seg[LIM_THREADS];
    __shared__ int64_t start[2];                                     // the file of the workgroup's first tile, and the tile's place in it
    constexpr int X6 = TRUE_PEAK ? 6 : 0;                            // samples the interpolation reaches past the halo of 2 H
    const int tid = threadIdx.x;
    const int E = LIM_TILE + 4 * hmax + 12;
    float *F0 = lds, *F1 = lds + E, *F2 = lds + 2 * E;
    double* scan = (double*)seg;                                     // the file search is over when the sums need it
    const int64_t u0 = (int64_t)blockIdx.x * total_tiles / gridDim.x, u1 = ((int64_t)blockIdx.x + 1) * total_tiles / gridDim.x;
    // where u0 lies: every thread counts the tiles of its slice of the table, the slice that holds u0 is walked by its thread
    const int per_thread = (nfiles + LIM_THREADS - 1) / LIM_THREADS;
    const int f_lo = (int)ld_min((int64_t)tid * per_thread, nfiles), f_hi = (int)ld_min((int64_t)f_lo + per_thread, nfiles);
    int64_t mine = 0;
    LimRow r;
    for (int f = f_lo; f < f_hi; ++f)
        if (lim_row(table + (int64_t)f * LD_COLS, total_in, hmax, &r)) mine += r.tiles;
    seg[tid] = mine;
    if (tid == 0) { start[0] = nfiles; start[1] = 0; }
    __syncthreads();
    int64_t before = 0;
    for (int i = 0; i < tid; ++i) before += seg[i];
    if (u0 >= before && u0 < before + mine) {
        int64_t at = before;
        for (int f = f_lo; f < f_hi; ++f) {
            const int64_t n = lim_row(table + (int64_t)f * LD_COLS, total_in, hmax, &r) ? r.tiles : 0;
            if (u0 < at + n) { start[0] = f; start[1] = u0 - at; break; }
            at += n;
        }
    }
    __syncthreads();
    int f = (int)start[0];
    int64_t off = start[1];
    float h[3][TP_TAPS];
    if (TRUE_PEAK) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int k = 0; k < TP_TAPS; ++k) h[p][k] = coef[p * TP_TAPS + k];
    }
    for (int64_t u = u0; u < u1 && f < nfiles; ++u, ++off) {
        bool ok = lim_row(table + (int64_t)f * LD_COLS, total_in, hmax, &r);
        while (!ok || off >= r.tiles) {                              // on to the next file that has a tile
            if (ok) off -= r.tiles;
            if (++f >= nfiles) return;                               // uniform: every thread walks the same rows
            ok = lim_row(table + (int64_t)f * LD_COLS, total_in, hmax, &r);
        }
        const int64_t t0 = off * LIM_TILE;                           // the tile's first sample; inside a tile every index is an int
        const int H = (int)r.H, W = 2 * H + 1, R = LIM_TILE + 4 * H, M = LIM_TILE + 2 * H, HL = 2 * H + X6;
        const float s = lim_s(stats, targets, f);
        // F0[i] = x[t0 - HL + i] for i < LIM_TILE + 2 HL, 0 outside [0, m); [va, vb): the samples that exist, from x[t0]
        const int va = t0 >= HL ? -HL : -(int)t0;
        const int64_t left = r.m - t0;
        const int vb = left < va ? va : (int)ld_min(left, LIM_TILE + HL);
        const int HLr = (HL + 3) & ~3, lines = (LIM_TILE + HL + HLr + 6) / 4;
        for (int64_t c = 0; c < r.ch; ++c) {
            const float* pt = planes + r.first + c * r.avail + t0;
            const int lead = (int)(((uintptr_t)pt >> 2) & 3);        // samples between the 16-byte line and x[t0]
            for (int g = tid; g < lines; g += LIM_THREADS) {
                const int j0 = 4 * g - lead - HLr;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (j0 >= va && j0 + 4 <= vb) {
                    const ragged_f32x4 q = *(const ragged_f32x4*)(pt + j0);
                    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (j0 + i >= va && j0 + i < vb) v[i] = pt[j0 + i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int at = j0 + i + HL;
                    if (at >= 0 && at < LIM_TILE + 2 * HL) F0[at] = v[i];
                }
            }
            __syncthreads();
            // F1[j] = max_c |x[t0 - 2 H + j]|; F2[j] = max_c max_q |point (t0 - 2 H - 1 + j) + q / 4|, which reads F0[j .. j + 12)
            for (int j = tid; j <= R; j += LIM_THREADS) {
                if (j < R) {
                    const float a = fabsf(F0[j + X6]);
                    F1[j] = c ? fmaxf(F1[j], a) : a;
                }
                if (TRUE_PEAK) {
                    float q = 0.f;
#pragma unroll
                    for (int ph = 0; ph < 3; ++ph) q = fmaxf(q, fabsf(tp_point(h[ph], F0 + j)));
                    F2[j] = c ? fmaxf(F2[j], q) : q;
                }
            }
            __syncthreads();
        }
        int over = 0;
        for (int j = tid; j < R; j += LIM_THREADS) {
            const int64_t t = t0 - 2 * H + j;
            float p = F1[j];
            if (TRUE_PEAK) p = fmaxf(p, fmaxf(F2[j], F2[j + 1]));    // the points on either side of t
            const float a = s * p;
            float rr = 1.f;
            if (t >= 0 && t < r.m && a > C) {
                rr = fmaxf((float)((double)C / (double)a), LIM_FLOOR);
                over = 1;
            }
            F0[j] = rr;
        }
        float gs[LIM_TILE / LIM_THREADS];                            // g * s of the samples t0 + tid + q LIM_THREADS
        if (__syncthreads_or(over)) {
            // B_k[j] = min r[j .. j + 2^k): K doublings, then the window of 2 H + 1 from j as two windows of 2^K
            const int K = 31 - __clz(W);
            float *src = F0, *dst = F1;
            for (int k = 0; k < K; ++k) {
                const int d = 1 << k;
                for (int j = tid; j < R; j += LIM_THREADS) dst[j] = fminf(src[j], src[j + d < R ? j + d : R - 1]);
                __syncthreads();
                float* t = src; src = dst; dst = t;
            }
            for (int j = tid; j < M; j += LIM_THREADS) F2[j] = fminf(src[j], src[j + W - (1 << K)]);      // mn[t0 - H + j]
            __syncthreads();
            // S[i] = mn[0] + .. + mn[i - 1] in float64 over F0 and F1: a thread sums a run, the runs are scanned, the run again
            double* S = (double*)lds;
            const int run = ((M + LIM_THREADS - 1) / LIM_THREADS) | 1;
            const int a0 = tid * run < M ? tid * run : M, a1 = a0 + run < M ? a0 + run : M;
            double sum = 0.0;
            for (int i = a0; i < a1; ++i) sum += (double)F2[i];
            scan[tid] = sum;
            __syncthreads();
            for (int d = 1; d < LIM_THREADS; d <<= 1) {
                const double t = tid >= d ? scan[tid - d] : 0.0;
                __syncthreads();
                scan[tid] += t;
                __syncthreads();
            }
            double acc = scan[tid] - sum;
            if (tid == 0) S[0] = 0.0;
            for (int i = a0; i < a1; ++i) {
                acc += (double)F2[i];
                S[i + 1] = acc;
            }
            __syncthreads();
            float gmin = 1.f;
            int count = 0;
#pragma unroll
            for (int q = 0; q < LIM_TILE / LIM_THREADS; ++q) {
                const int l = tid + q * LIM_THREADS;
                const float g = (float)((S[l + W] - S[l]) / (double)W);
                const bool inside = t0 + l < r.m;
                gs[q] = inside ? g * s : 1.f;
                if (inside && g < 1.f) { gmin = fminf(gmin, g); ++count; }
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                gmin = fminf(gmin, __shfl_xor(gmin, d));
                count += __shfl_xor(count, d);
            }
            if ((tid & 63) == 0 && count > 0) {
                atomicMin((unsigned long long*)(rows + (int64_t)f * 4 + 1), (unsigned long long)__double_as_longlong((double)gmin));
                atomicAdd((unsigned long long*)(rows + (int64_t)f * 4 + 2), (unsigned long long)count);
            }
        } else {
#pragma unroll
            for (int q = 0; q < LIM_TILE / LIM_THREADS; ++q) gs[q] = t0 + tid + q * LIM_THREADS < r.m ? s : 1.f;
        }
#pragma unroll
        for (int q = 0; q < LIM_TILE / LIM_THREADS; ++q) F2[tid + q * LIM_THREADS] = gs[q];      // mn was last read before a barrier
        __syncthreads();
        // y = x * (g * s): whole 16-byte lines of the OUTPUT plane where they lie inside the tile, read as one where the input lies alike
        const int n = (int)ld_min(r.avail - t0, LIM_TILE);
        for (int64_t c = 0; c < r.ch; ++c) {
            const float* pi = planes + r.first + c * r.avail + t0;
            float* po = out + r.first + c * r.avail + t0;
            const int lead = (int)(((uintptr_t)po >> 2) & 3);
            const bool alike = (((uintptr_t)pi ^ (uintptr_t)po) & 15) == 0;
            for (int g = tid; g < (n + lead + 3) / 4; g += LIM_THREADS) {
                const int j0 = 4 * g - lead;
                if (alike && j0 >= 0 && j0 + 4 <= n) {
                    ragged_f32x4 v = *(const ragged_f32x4*)(pi + j0);
                    v[0] *= F2[j0]; v[1] *= F2[j0 + 1]; v[2] *= F2[j0 + 2]; v[3] *= F2[j0 + 3];
                    *(ragged_f32x4*)(po + j0) = v;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (j0 + i >= 0 && j0 + i < n) po[j0 + i] = pi[j0 + i] * F2[j0 + i];
                }
            }
        }
        __syncthreads();                                             // the next tile overwrites the arrays
    }
}

template <bool TRUE_PEAK, typename... Args>
static int lim_launch(const char* who, unsigned grid, int hmax, hipStream_t st, const Args&... args) {
    static sos_device_once attr_once;
    if (sos_per_device_once(attr_once, [who] {
            if (hipFuncSetAttribute((const void*)lim_kernel<TRUE_PEAK>, hipFuncAttributeMaxDynamicSharedMemorySize, LIM_LDS(LIM_MAX_H)) !=
                hipSuccess) {
                sos_set_error("%s: cannot raise the dynamic LDS limit", who);
                return (int)SOS_ELAUNCH;
            }
            return (int)SOS_OK;
        }))
        return SOS_ELAUNCH;
    hipLaunchKernelGGL(lim_kernel<TRUE_PEAK>, dim3(grid), dim3(LIM_THREADS), (size_t)LIM_LDS(hmax), st, args...);
    return SOS_OK;
}

extern "C" int sos_limiter_batch_f32(const float* planes, float* out, const int64_t* table, const int64_t* table_host, int nfiles,
                                     const double* stats, const double* targets, double ceiling_db, int true_peak, const float* coef,
                                     double* rows, sos_stream_t stream) {
    const char* who = "sos_limiter_batch_f32";
    LdTotals t;
    const int rc = ld_args(who, !planes || !out || !table || !table_host || !stats || !targets || !rows || (true_peak && !coef),
                           table_host, nfiles, 1, false, &t);
    if (rc != SOS_OK) return rc;
    if (!(ceiling_db <= 0.0) || !std::isfinite(ceiling_db)) {
        sos_set_error("%s: the ceiling is a finite level of at most 0 dBFS, got %g", who, ceiling_db);
        return SOS_EINVAL;
    }
    if (planes + t.in > out && out + t.in > planes) {
        sos_set_error("%s: the output overlaps the planes (the limiter works out of place)", who);
        return SOS_EINVAL;
    }
    int64_t tiles = 0, hmax = 1;
    for (int f = 0; f < nfiles; ++f) {
        const int64_t H = table_host[(int64_t)f * LD_COLS + 4];
        if (H < 1 || H > LIM_MAX_H) {
            sos_set_error("%s: file %d has a look-ahead of %lld samples (1 .. %d)", who, f, (long long)H, LIM_MAX_H);
            return SOS_EINVAL;
        }
        hmax = std::max(hmax, H);
    }
    for (int f = 0; f < nfiles; ++f) {
        LimRow r;
        if (lim_row(table_host + (int64_t)f * LD_COLS, t.in, hmax, &r)) tiles += r.tiles;
    }
    hipStream_t st = (hipStream_t)stream;
    const float C = (float)pow(10.0, ceiling_db / 20.0);
    const dim3 per_file((unsigned)((nfiles + MT - 1) / MT));
    hipLaunchKernelGGL(lim_init_kernel, per_file, dim3(MT), 0, st, table, nfiles, t.in, (int)hmax, stats, targets, rows);
    if (tiles > 0) {
        const unsigned grid = ragged_grid(tiles, 1, LIM_MAX_GRID);
        const int lrc = true_peak ? lim_launch<true>(who, grid, (int)hmax, st, planes, out, table, nfiles, t.in, tiles, (int)hmax, stats,
                                                     targets, C, coef, rows)
                                  : lim_launch<false>(who, grid, (int)hmax, st, planes, out, table, nfiles, t.in, tiles, (int)hmax, stats,
                                                      targets, C, coef, rows);
        if (lrc != SOS_OK) return lrc;
    }
    hipLaunchKernelGGL(lim_finish_kernel, per_file, dim3(MT), 0, st, table, nfiles, t.in, (int)hmax, rows);
    return sos_check_launch(who);
}
