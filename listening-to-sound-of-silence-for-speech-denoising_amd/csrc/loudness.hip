// loudness.hip -- ITU-R BS.1770 / EBU R128 integrated loudness of a group of files, and the gain that brings each to a target,
// on the f32 channel planes the encode reads (metrics.loudness_batch / audio_io.loudness_gain_batch_device; float64 restatement:
// tests/loudness_reference.py).  sos_loudness_batch_f64 is one launch sequence, sos_loudness_gain_batch_f32 one launch; neither
// waits for the device.
// The K-weighting filter (two biquads, transposed direct form II, zero initial state) is a linear recurrence on a state of four
// doubles: s' = A s + B x.  A plane is cut into CHUNKS that never straddle a 100 ms hop (a hop of h samples holds `split` chunks,
// chunk s of it = samples [s h / split, (s + 1) h / split), so every chunk is lc = h / split or lc + 1 samples long), and:
//   loud_chunk_kernel<false>  one thread per chunk runs the filter from ZERO state: the state it ends in, and max |x|
//   loud_carry_kernel         one thread per plane: the state every chunk really starts from, s[q + 1] = A^len(q) s[q] + end[q];
//                             A^lc comes from running the four unit states through lc steps of silence, A^(lc + 1) is one step more
//   loud_chunk_kernel<true>   the chunks again from their true state, summing y^2 per chunk
//   loud_gate_kernel          one workgroup per file: a 400 ms block = 4 split consecutive chunk sums; channels weighted and added;
//                             the absolute and the relative gate; {L, sample peak, blocks passing, blocks absolutely gated}
// A thread walks consecutive samples, so adjacent lanes are a chunk apart: the 64 chunks of a wave are staged through LDS 32
// samples at a time -- a half wave loads the 128 contiguous bytes of one chunk, a lane then reads its own row (33 floats apart:
// no bank is hit twice).  Everything after the load is float64.  All sums are taken in a fixed order: two calls give equal bits.
// Bounds: the rule of ragged.h, as pcm_io.hip applies it -- the host refuses a row of table_host outside the totals it summed
// (SOS_EINVAL, naming the file), the kernels skip a row of the DEVICE table that fails the same rule; the row rule and the host's
// checks stand in loudness_core.h, which limiter.hip shares.
// Below the gain: the other EBU R128 measures on the same table -- sos_true_peak_batch_f64 (the true peak by 4x interpolation,
// float32, a flat grid over the tiles of all planes) and sos_loudness_range_batch_f64 (loudness range and the maximum momentary /
// short-term loudness, from the chunk energies of the work buffer); float64 restatement: tests/r128_reference.py.
#include "loudness_core.h"
#include <math.h>

#define LD_TILE 32                      // samples per chunk staged at a time
#define LD_MAX_GRID 4096
#define LD_CARRY 8                      // chunk states the carry fetches ahead of its recurrence
#define LD_WORK 6                       // f64 arrays of the work buffer, one entry per chunk: state[4], energy, peak
#define LD_GAIN_THREADS 256
#define LD_GAIN_MAX_GRID 1024

// samples [a, b) of chunk q (both cut at the file's frames), and whether it is one of the longer chunks of its hop
__device__ __forceinline__ void ld_chunk(const LdRow& r, int split, int64_t q, int64_t* a, int64_t* b) {
    const int64_t hop = q / split, s = q - hop * split;
    *a = ld_min(hop * r.h + s * r.h / split, r.frames);
    *b = ld_min(hop * r.h + (s + 1) * r.h / split, r.frames);
}

struct LdFilter { double b10, b11, b12, a11, a12, b20, b21, b22, a21, a22; };
struct LdState { double s1, s2, t1, t2; };
__device__ __forceinline__ LdFilter ld_filter(const double* c) { return {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9]}; }
// one sample through both biquads (transposed direct form II)
__device__ __forceinline__ double ld_step(const LdFilter& k, LdState& s, double x) {
    const double u = k.b10 * x + s.s1;
    s.s1 = k.b11 * x - k.a11 * u + s.s2;
    s.s2 = k.b12 * x - k.a12 * u;
    const double y = k.b20 * u + s.t1;
    s.t1 = k.b21 * u - k.a21 * y + s.t2;
    s.t2 = k.b22 * u - k.a22 * y;
    return y;
}

template <bool ENERGY>
__global__ __launch_bounds__(LD_WAVE) void loud_chunk_kernel(const float* __restrict__ planes, const int64_t* __restrict__ table,
                                                             const double* __restrict__ coef, int split, int64_t total_in,
                                                             int64_t total_ch, int64_t total_chunks, double* __restrict__ work) {
    __shared__ float tile[LD_WAVE][LD_TILE + 1];
    __shared__ int64_t lo[LD_WAVE];
    __shared__ int64_t len[LD_WAVE];
    LdRow r;
    if (!ld_row(table + (int64_t)blockIdx.y * LD_COLS, split, total_in, total_ch, total_chunks, &r)) return;
    const LdFilter k = ld_filter(coef + (int64_t)blockIdx.y * 10);
    const int tid = threadIdx.x;
    const int64_t groups = (r.nq + LD_WAVE - 1) / LD_WAVE, longest = r.h / split + 1;
    for (int64_t u = blockIdx.x; u < groups * r.ch; u += gridDim.x) {
        const int64_t c = u / groups, q = (u - c * groups) * LD_WAVE + tid;
        const bool live = q < r.nq;
        int64_t a = 0, b = 0;
        if (live) ld_chunk(r, split, q, &a, &b);
        const int64_t n = b - a, at = r.qoff + c * r.nq + q;
        lo[tid] = a;
        len[tid] = n;
        const float* p = planes + r.first + c * r.avail;
        LdState s = {0.0, 0.0, 0.0, 0.0};
        if (ENERGY && live) s = {work[at], work[total_chunks + at], work[2 * total_chunks + at], work[3 * total_chunks + at]};
        double acc = 0.0;
        float pk = 0.f;
        __syncthreads();
        for (int64_t t0 = 0; t0 < longest; t0 += LD_TILE) {
            const int col = tid & (LD_TILE - 1);
            for (int row = tid / LD_TILE; row < LD_WAVE; row += LD_WAVE / LD_TILE) {
                const int64_t i = lo[row] + t0 + col;                // zero from the plane's end on, as the encode reads it
                tile[row][col] = (t0 + col < len[row] && i < r.avail) ? p[i] : 0.f;
            }
            __syncthreads();
            const int m = (int)ld_min(LD_TILE, n - t0);
            for (int j = 0; j < m; ++j) {
                const float x = tile[tid][j];
                const double y = ld_step(k, s, (double)x);
                if (ENERGY) acc += y * y; else pk = fmaxf(pk, fabsf(x));
            }
            __syncthreads();
        }
        if (live) {
            if (ENERGY) {
                work[4 * total_chunks + at] = acc;
            } else {
                work[at] = s.s1; work[total_chunks + at] = s.s2; work[2 * total_chunks + at] = s.t1; work[3 * total_chunks + at] = s.t2;
                work[5 * total_chunks + at] = (double)pk;
            }
        }
    }
}

// Thread c of workgroup f: plane c of file f.  m[j] = what the unit state j has become after lc samples of silence, i.e. column
// j of A^lc; one more step gives A^(lc + 1).  Then the chunks in order: the zero-state end of chunk q is replaced by the state
// the chunk starts from.  The loads of LD_CARRY chunks are issued ahead of the recurrence that needs them.
__global__ __launch_bounds__(LD_WAVE) void loud_carry_kernel(const int64_t* __restrict__ table, const double* __restrict__ coef, int split,
                                                             int64_t total_in, int64_t total_ch, int64_t total_chunks,
                                                             double* __restrict__ work) {
    LdRow r;
    if (!ld_row(table + (int64_t)blockIdx.y * LD_COLS, split, total_in, total_ch, total_chunks, &r)) return;
    if ((int64_t)threadIdx.x >= r.ch) return;
    const LdFilter k = ld_filter(coef + (int64_t)blockIdx.y * 10);
    const int64_t lc = r.h / split;
    LdState m0[4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}}, m1[4];
    for (int64_t i = 0; i < lc; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ld_step(k, m0[j], 0.0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m1[j] = m0[j];
        ld_step(k, m1[j], 0.0);
    }
    double* w0 = work + r.qoff + (int64_t)threadIdx.x * r.nq;
    LdState s = {0.0, 0.0, 0.0, 0.0};
    int64_t sub = 0;                                                 // the chunk's place in its hop
    for (int64_t q0 = 0; q0 < r.nq; q0 += LD_CARRY) {
        LdState e[LD_CARRY];
#pragma unroll
        for (int j = 0; j < LD_CARRY; ++j) {
            const int64_t q = ld_min(q0 + j, r.nq - 1);
            e[j] = {w0[q], w0[total_chunks + q], w0[2 * total_chunks + q], w0[3 * total_chunks + q]};
        }
#pragma unroll
        for (int j = 0; j < LD_CARRY; ++j) {
            const int64_t q = q0 + j;
            if (q < r.nq) {
                w0[q] = s.s1; w0[total_chunks + q] = s.s2; w0[2 * total_chunks + q] = s.t1; w0[3 * total_chunks + q] = s.t2;
                const bool longer = (sub + 1) * r.h / split - sub * r.h / split != lc;
                LdState m[4], t;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    m[i] = {longer ? m1[i].s1 : m0[i].s1, longer ? m1[i].s2 : m0[i].s2, longer ? m1[i].t1 : m0[i].t1,
                            longer ? m1[i].t2 : m0[i].t2};
                t.s1 = e[j].s1 + m[0].s1 * s.s1 + m[1].s1 * s.s2 + m[2].s1 * s.t1 + m[3].s1 * s.t2;
                t.s2 = e[j].s2 + m[0].s2 * s.s1 + m[1].s2 * s.s2 + m[2].s2 * s.t1 + m[3].s2 * s.t2;
                t.t1 = e[j].t1 + m[0].t1 * s.s1 + m[1].t1 * s.s2 + m[2].t1 * s.t1 + m[3].t1 * s.t2;
                t.t2 = e[j].t2 + m[0].t2 * s.s1 + m[1].t2 * s.s2 + m[2].t2 * s.t1 + m[3].t2 * s.t2;
                s = t;
                if (++sub == split) sub = 0;
            }
        }
    }
}

// Workgroup f: file f.  z of block j = sum over channels of weight * (the 4 split chunk sums from chunk j split on) / (4 h).
__global__ __launch_bounds__(MT) void loud_gate_kernel(const int64_t* __restrict__ table, const double* __restrict__ weights, int split,
                                                       int64_t total_in, int64_t total_ch, int64_t total_chunks,
                                                       const double* __restrict__ work, double* __restrict__ stats) {
    __shared__ double red[MT];
    double* out = stats + (int64_t)blockIdx.x * 4;
    LdRow r;
    if (!ld_row(table + (int64_t)blockIdx.x * LD_COLS, split, total_in, total_ch, total_chunks, &r)) {
        if (threadIdx.x == 0) { out[0] = NAN; out[1] = NAN; out[2] = -1.0; out[3] = -1.0; }
        return;
    }
    const int64_t blocks = r.frames >= 4 * r.h ? (r.frames - 4 * r.h) / r.h + 1 : 0;
    const double* energy = work + 4 * total_chunks + r.qoff;
    const double* peaks = work + 5 * total_chunks + r.qoff;
    const double* w = weights + r.woff;
    const double per = 4.0 * (double)r.h;
    auto block_z = [&](int64_t j) {
        double z = 0.0;
        for (int64_t c = 0; c < r.ch; ++c) {
            const double* e = energy + c * r.nq + j * split;
            double sum = 0.0;
            for (int i = 0; i < 4 * split; ++i) sum += e[i];
            z += w[c] * (sum / per);
        }
        return z;
    };
    double pk = 0.0;
    for (int64_t i = threadIdx.x; i < r.nq * r.ch; i += MT) pk = fmax(pk, peaks[i]);
    pk = block_max(pk, red);
    double sum = 0.0, count = 0.0;
    for (int64_t j = threadIdx.x; j < blocks; j += MT) {
        const double z = block_z(j);
        if (-0.691 + 10.0 * log10(z) > -70.0) { sum += z; count += 1.0; }
    }
    sum = block_sum(sum, red);
    const double n_abs = block_sum(count, red);
    const double gate = -0.691 + 10.0 * log10(sum / n_abs) - 10.0;      // NaN without a block: nothing passes it
    sum = 0.0; count = 0.0;
    for (int64_t j = threadIdx.x; j < blocks; j += MT) {
        const double z = block_z(j), l = -0.691 + 10.0 * log10(z);
        if (l > -70.0 && l > gate) { sum += z; count += 1.0; }
    }
    sum = block_sum(sum, red);
    const double n_rel = block_sum(count, red);
    if (threadIdx.x == 0) {
        out[0] = n_rel > 0.0 ? -0.691 + 10.0 * log10(sum / n_rel) : -INFINITY;
        out[1] = pk;
        out[2] = n_rel;
        out[3] = n_abs;
    }
}

// g = min(10^((T - L) / 20), 10^(P / 20) / peak) in double, 1 where L, T or the peak give none; every thread of file f derives
// it from the file's row.  A thread owns four samples that lie on one 16-byte line of its plane wherever the plane starts.
__global__ __launch_bounds__(LD_GAIN_THREADS) void loud_gain_kernel(float* __restrict__ planes, const int64_t* __restrict__ table,
                                                                    int64_t total_in, const double* __restrict__ stats,
                                                                    const double* __restrict__ targets, double ceiling_db,
                                                                    float* __restrict__ gains, int* __restrict__ limited) {
    const int64_t* te = table + (int64_t)blockIdx.y * LD_COLS;
    const int64_t first = te[0], avail = te[1], ch = te[2], frames = te[3];
    const double L = stats[(int64_t)blockIdx.y * 4], peak = stats[(int64_t)blockIdx.y * 4 + 1], T = targets[blockIdx.y];
    double g64 = 1.0;
    int bound = 0;
    if (isfinite(L) && isfinite(T) && isfinite(peak) && peak > 0.0) {
        const double to_target = pow(10.0, (T - L) / 20.0), to_ceiling = pow(10.0, ceiling_db / 20.0) / peak;
        bound = to_ceiling < to_target;
        g64 = bound ? to_ceiling : to_target;
    }
    const float g = (float)g64;
    if (blockIdx.x == 0 && threadIdx.x == 0) { gains[blockIdx.y] = g; limited[blockIdx.y] = bound; }
    if (!ld_planes_inside(first, avail, ch, total_in) || frames < 0) return;
    const int64_t m = ld_min(frames, avail);                           // samples past the frames the file is written with stay
    for (int64_t c = 0; c < ch; ++c) {
        float* p = planes + first + c * avail;
        const int64_t lead = (int64_t)(((uintptr_t)p >> 2) & 3);     // samples between the 16-byte line and the plane's start
        const int64_t units = (m + lead + 3) / 4;
        for (int64_t u = (int64_t)blockIdx.x * LD_GAIN_THREADS + threadIdx.x; u < units; u += (int64_t)gridDim.x * LD_GAIN_THREADS) {
            const int64_t j0 = 4 * u - lead;
            if (j0 >= 0 && j0 + 4 <= m) {
                ragged_f32x4 v = *(ragged_f32x4*)(p + j0);
                v[0] *= g; v[1] *= g; v[2] *= g; v[3] *= g;
                *(ragged_f32x4*)(p + j0) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j0 + i >= 0 && j0 + i < m) p[j0 + i] *= g;
            }
        }
    }
}

extern "C" int64_t sos_loudness_workspace_bytes(const int64_t* table_host, int nfiles, int split) {
    LdTotals t;
    if (ld_args("sos_loudness_workspace_bytes", false, table_host, nfiles, split, true, &t) != SOS_OK) return -1;
    return (int64_t)align256((size_t)std::max<int64_t>(t.chunks, 1) * LD_WORK * sizeof(double));
}

extern "C" int sos_loudness_batch_f64(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles,
                                      const double* coef, const double* weights, int split, void* work, int64_t work_bytes,
                                      double* stats, sos_stream_t stream) {
    const char* who = "sos_loudness_batch_f64";
    LdTotals t;
    const int rc = ld_args(who, !planes || !table || !table_host || !coef || !weights || !work || !stats, table_host, nfiles, split, true, &t);
    if (rc != SOS_OK) return rc;
    const int64_t need = (int64_t)align256((size_t)std::max<int64_t>(t.chunks, 1) * LD_WORK * sizeof(double));
    if (work_bytes < need) {
        sos_set_error("%s: the work buffer holds %lld bytes, %lld chunks need %lld", who, (long long)work_bytes, (long long)t.chunks,
                      (long long)need);
        return SOS_ENOSPC;
    }
    hipStream_t st = (hipStream_t)stream;
    double* w = (double*)work;
    const dim3 grid(ragged_grid(t.units, 1, LD_MAX_GRID), (unsigned)nfiles);
    hipLaunchKernelGGL(loud_chunk_kernel<false>, grid, dim3(LD_WAVE), 0, st, planes, table, coef, split, t.in, t.ch, t.chunks, w);
    hipLaunchKernelGGL(loud_carry_kernel, dim3(1, (unsigned)nfiles), dim3(LD_WAVE), 0, st, table, coef, split, t.in, t.ch, t.chunks, w);
    hipLaunchKernelGGL(loud_chunk_kernel<true>, grid, dim3(LD_WAVE), 0, st, planes, table, coef, split, t.in, t.ch, t.chunks, w);
    hipLaunchKernelGGL(loud_gate_kernel, dim3((unsigned)nfiles), dim3(MT), 0, st, table, weights, split, t.in, t.ch, t.chunks, w, stats);
    return sos_check_launch(who);
}

extern "C" int sos_loudness_gain_batch_f32(float* planes, const int64_t* table, const int64_t* table_host, int nfiles,
                                           const double* stats, const double* targets, double ceiling_db, float* gains,
                                           int* limited, sos_stream_t stream) {
    const char* who = "sos_loudness_gain_batch_f32";
    LdTotals t;
    const int rc = ld_args(who, !planes || !table || !table_host || !stats || !targets || !gains || !limited, table_host, nfiles, 1, false, &t);
    if (rc != SOS_OK) return rc;
    if (!(ceiling_db <= 0.0)) {
        sos_set_error("%s: the ceiling is at most 0 dBFS, got %g", who, ceiling_db);
        return SOS_EINVAL;
    }
    const dim3 grid(ragged_grid((t.longest + 3) / 4 + 1, LD_GAIN_THREADS, LD_GAIN_MAX_GRID), (unsigned)nfiles);
    hipLaunchKernelGGL(loud_gain_kernel, grid, dim3(LD_GAIN_THREADS), 0, (hipStream_t)stream, planes, table, t.in, stats, targets,
                       ceiling_db, gains, limited);
    return sos_check_launch(who);
}

// ---- the true peak of a group of files (ITU-R BS.1770-4 Annex 2 by the project's own interpolator; tests/r128_reference.py)
// 4x oversampling by a 48-tap polyphase windowed sinc: the point n + p / 4 (p = 1, 2, 3) is v = sum_{k = -5 .. 6} h_p[k] x[n + k],
// 12 fmaf in tap order in float32, for n = -1 .. frames - 1; phase 0 is the sample itself.  The true peak of a file is the
// maximum of |x| and |v| over its channels.  Samples outside [0, min(frames, available)) read 0, so nothing past n = that end
// + 4 can differ from 0 and the points stop there.
//   tp_init_kernel   peaks[f] = 0, or NaN for a row outside the totals
//   tp_peak_kernel   a FLAT grid over the tiles of all planes of all files: workgroup b owns the tiles [b T / G, (b + 1) T / G)
//                    of the T the host counted, finds the file of its first tile once (256 threads sum the tile counts of a
//                    slice of the table each) and walks on from there, so one long file and many short ones fill the chip alike.
//                    A tile is TP_TILE points of one plane: its TP_TILE + 11 samples are staged in LDS from the 16-byte lines of
//                    the plane (wherever it starts: `lead`, as loud_gain_kernel), a lane reads the 19 consecutive samples of its
//                    8 points once (5 16-byte LDS reads) and slides a register window over them, the three phases sharing it.
//                    The lane maxima meet in a wave, the waves in an atomic maximum on the bits of the non-negative double:
//                    a maximum has no order, two calls give equal bits.
#define TP_THREADS 256
#define TP_POINTS 8                     // consecutive points of a lane
#define TP_TILE (TP_THREADS * TP_POINTS)
#define TP_HALO (TP_TAPS - 1)
#define TP_LDS (TP_TILE + 16)           // the samples of a tile, its halo, and what the last lane's fifth 16-byte read covers
#define TP_MAX_GRID 2048

struct TpRow { int64_t first, avail, ch, m, points, tiles; };    // m: samples that count; points n = -1 .. points - 2; tiles per plane

// the rule for a row of the true peak: the planes inside the total; a file without a sample has no tile and reads 0
__host__ __device__ static inline bool tp_row(const int64_t* te, int64_t total_in, TpRow* r) {
    *r = {te[0], te[1], te[2], 0, 0, 0};
    const int64_t frames = te[3];
    if (!ld_planes_inside(r->first, r->avail, r->ch, total_in) || frames < 0) return false;
    r->m = ld_min(frames, r->avail);
    r->points = r->m ? ld_min(frames, r->m + 5) + 1 : 0;
    r->tiles = (r->points + TP_TILE - 1) / TP_TILE;
    return true;
}

__global__ void tp_init_kernel(const int64_t* __restrict__ table, int nfiles, int64_t total_in, double* __restrict__ peaks) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nfiles) return;
    TpRow r;
    peaks[f] = tp_row(table + (int64_t)f * LD_COLS, total_in, &r) ? 0.0 : (double)NAN;
}

__global__ __launch_bounds__(TP_THREADS) void tp_peak_kernel(const float* __restrict__ planes, const int64_t* __restrict__ table,
                                                             int nfiles, int64_t total_in, int64_t total_tiles,
                                                             const float* __restrict__ coef, double* __restrict__ peaks) {
    __shared__ __attribute__((aligned(16))) float s[TP_LDS];
    __shared__ int64_t seg[TP_THREADS];
    __shared__ int64_t start[2];                                     // the file of the workgroup's first tile, and the tile's place in it
    const int tid = threadIdx.x;
    const int64_t u0 = (int64_t)blockIdx.x * total_tiles / gridDim.x, u1 = ((int64_t)blockIdx.x + 1) * total_tiles / gridDim.x;
    // where u0 lies: every thread counts the tiles of its slice of the table, the slice that holds u0 is walked by its thread
    const int per = (nfiles + TP_THREADS - 1) / TP_THREADS;
    const int f_lo = ld_min((int64_t)tid * per, nfiles), f_hi = ld_min((int64_t)f_lo + per, nfiles);
    int64_t mine = 0;
    TpRow r;
    for (int f = f_lo; f < f_hi; ++f)
        if (tp_row(table + (int64_t)f * LD_COLS, total_in, &r)) mine += r.ch * r.tiles;
    seg[tid] = mine;
    if (tid == 0) { start[0] = nfiles; start[1] = 0; }
    __syncthreads();
    int64_t before = 0;
    for (int i = 0; i < tid; ++i) before += seg[i];
    if (u0 >= before && u0 < before + mine) {
        int64_t at = before;
        for (int f = f_lo; f < f_hi; ++f) {
            const int64_t n = tp_row(table + (int64_t)f * LD_COLS, total_in, &r) ? r.ch * r.tiles : 0;
            if (u0 < at + n) { start[0] = f; start[1] = u0 - at; break; }
            at += n;
        }
    }
    __syncthreads();
    int f = (int)start[0];
    int64_t off = start[1];
    float h[3][TP_TAPS];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int k = 0; k < TP_TAPS; ++k) h[p][k] = coef[p * TP_TAPS + k];
    for (int64_t u = u0; u < u1 && f < nfiles; ++u, ++off) {
        bool ok = tp_row(table + (int64_t)f * LD_COLS, total_in, &r);
        while (!ok || off >= r.ch * r.tiles) {                       // on to the next file that has a tile
            if (ok) off -= r.ch * r.tiles;
            if (++f >= nfiles) return;                               // uniform: every thread walks the same rows
            ok = tp_row(table + (int64_t)f * LD_COLS, total_in, &r);
        }
        const int64_t c = off / r.tiles, m0 = (off - c * r.tiles) * TP_TILE;       // the tile's first point is n = m0 - 1
        const float* pt = planes + r.first + c * r.avail + m0;        // x[m0]: inside a tile every index is an int from here
        // s[i] = x[m0 - 6 + i] for i < TP_TILE + 11, 0 outside [0, m): whole 16-byte lines of the plane where they lie inside.
        // [va, vb): the samples that exist, from x[m0]; line g starts at j0 = 4 g - lead - 8 <= -8, line 515 reaches x[m0 + TP_TILE + 4]
        const int va = m0 >= 6 ? -6 : -(int)m0, vb = (int)ld_min(r.m - m0, TP_TILE + 6);
        const int lead = (int)(((uintptr_t)pt >> 2) & 3);
#pragma unroll
        for (int g = tid; g < (TP_TILE + TP_HALO + 8) / 4; g += TP_THREADS) {
            const int j0 = 4 * g - lead - 8;
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
                const int at = j0 + i + 6;
                if (at >= 0 && at < TP_TILE + TP_HALO) s[at] = v[i];
            }
        }
        __syncthreads();
        float w[TP_POINTS + TP_HALO + 1];                            // 20 samples from the lane's first: the 19 of its window and one more
#pragma unroll
        for (int i = 0; i < (TP_POINTS + TP_HALO + 1) / 4; ++i) {
            const ragged_f32x4 q = *(const ragged_f32x4*)(s + tid * TP_POINTS + 4 * i);
            w[4 * i] = q[0]; w[4 * i + 1] = q[1]; w[4 * i + 2] = q[2]; w[4 * i + 3] = q[3];
        }
        float pk = 0.f;
        const int left = (int)ld_min(r.points - m0, TP_TILE) - tid * TP_POINTS;    // points of the plane from the lane's first on
#pragma unroll
        for (int j = 0; j < TP_POINTS; ++j) {
            float best = fabsf(w[j + 5]);                            // the sample x[n] itself; n = -1 reads the 0 before the plane
#pragma unroll
            for (int ph = 0; ph < 3; ++ph) best = fmaxf(best, fabsf(tp_point(h[ph], w + j)));
            if (j < left) pk = fmaxf(pk, best);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d));
        if ((tid & 63) == 0 && pk > 0.f)
            atomicMax((unsigned long long*)(peaks + f), (unsigned long long)__double_as_longlong((double)pk));
        __syncthreads();                                             // the next tile overwrites s
    }
}

extern "C" int sos_true_peak_batch_f64(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles,
                                       const float* coef, double* peaks, sos_stream_t stream) {
    const char* who = "sos_true_peak_batch_f64";
    LdTotals t;
    const int rc = ld_args(who, !planes || !table || !table_host || !coef || !peaks, table_host, nfiles, 1, false, &t);
    if (rc != SOS_OK) return rc;
    int64_t tiles = 0;
    for (int f = 0; f < nfiles; ++f) {
        TpRow r;
        if (tp_row(table_host + (int64_t)f * LD_COLS, t.in, &r)) tiles += r.ch * r.tiles;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tp_init_kernel, dim3((unsigned)((nfiles + MT - 1) / MT)), dim3(MT), 0, st, table, nfiles, t.in, peaks);
    if (tiles > 0)
        hipLaunchKernelGGL(tp_peak_kernel, dim3(ragged_grid(tiles, 1, TP_MAX_GRID)), dim3(TP_THREADS), 0, st, planes, table, nfiles,
                           t.in, tiles, coef, peaks);
    return sos_check_launch(who);
}

// ---- loudness range (EBU Tech 3342) and the maximum momentary / short-term loudness, from the chunk energies the measurement
// left in its work buffer (tests/r128_reference.py).  range_work: f64 [2][H] with H = total chunks / split, the hops of all planes;
// file f owns [qoff / split, + its whole hops) of either half.
//   range_hops_kernel   one thread per whole hop: e[i] = sum_c w_c (the hop's `split` chunk sums, in order)
//   range_gate_kernel   one workgroup per file: z_st[j] = (e[j] + .. + e[j + 29]) / (30 h) in order, the absolute gate l > -70 and
//                       the relative gate l > (loudness of the mean z_st of the absolutely gated windows) - 20 as loud_gate_kernel
//                       applies its own; a window that fails one is marked -1.  The two nearest-rank percentiles are SELECTED,
//                       not sorted: the bits of a positive double order as an integer, so the value of rank k is the largest
//                       P with (windows below P) <= k, built bit by bit in 63 counting passes, both ranks in one pass.
#define LR_WINDOW 30

struct LrRow { int64_t hoff, nh, windows; };
__device__ __forceinline__ LrRow lr_row(const LdRow& r, int split) {
    const int64_t nh = r.frames / r.h;
    return {r.qoff / split, nh, nh >= LR_WINDOW ? nh - LR_WINDOW + 1 : 0};
}

__global__ __launch_bounds__(MT) void range_hops_kernel(const int64_t* __restrict__ table, const double* __restrict__ weights, int split,
                                                        int64_t total_in, int64_t total_ch, int64_t total_chunks,
                                                        const double* __restrict__ work, double* __restrict__ range_work) {
    LdRow r;
    if (!ld_row(table + (int64_t)blockIdx.y * LD_COLS, split, total_in, total_ch, total_chunks, &r)) return;
    const LrRow q = lr_row(r, split);
    const double* energy = work + 4 * total_chunks + r.qoff;
    const double* w = weights + r.woff;
    for (int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x; i < q.nh; i += (int64_t)gridDim.x * MT) {
        double e = 0.0;
        for (int64_t c = 0; c < r.ch; ++c) {
            const double* ec = energy + c * r.nq + i * split;
            double sum = 0.0;
            for (int k = 0; k < split; ++k) sum += ec[k];
            e += w[c] * sum;
        }
        range_work[q.hoff + i] = e;
    }
}

__device__ __forceinline__ double lr_loudness(double z) { return -0.691 + 10.0 * log10(z); }

__global__ __launch_bounds__(MT) void range_gate_kernel(const int64_t* __restrict__ table, int split, int64_t total_in, int64_t total_ch,
                                                        int64_t total_chunks, double* __restrict__ range_work, double* __restrict__ out4) {
    __shared__ double red[MT];
    double* out = out4 + (int64_t)blockIdx.x * 4;
    LdRow r;
    if (!ld_row(table + (int64_t)blockIdx.x * LD_COLS, split, total_in, total_ch, total_chunks, &r)) {
        if (threadIdx.x == 0) { out[0] = NAN; out[1] = NAN; out[2] = NAN; out[3] = -1.0; }
        return;
    }
    const LrRow q = lr_row(r, split);
    const int64_t total_hops = total_chunks / split;
    const double* e = range_work + q.hoff;
    double* zw = range_work + total_hops + q.hoff;
    // the maximum momentary loudness: a 400 ms block is four hops
    const int64_t blocks = q.nh >= 4 ? q.nh - 3 : 0;
    double best = -1.0;
    for (int64_t j = threadIdx.x; j < blocks; j += MT) best = fmax(best, (e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / (4.0 * (double)r.h));
    const double z_m = block_max(best, red);
    // the windows, their maximum and the absolute gate
    const double per = (double)LR_WINDOW * (double)r.h;
    double sum = 0.0, count = 0.0;
    best = -1.0;
    for (int64_t j = threadIdx.x; j < q.windows; j += MT) {
        double z = 0.0;
        for (int i = 0; i < LR_WINDOW; ++i) z += e[j + i];
        z /= per;
        zw[j] = z;
        best = fmax(best, z);
        if (lr_loudness(z) > -70.0) { sum += z; count += 1.0; }
    }
    const double z_st = block_max(best, red);
    sum = block_sum(sum, red);
    const double n_abs = block_sum(count, red);
    const double gate = lr_loudness(sum / n_abs) - 20.0;               // NaN without a window: nothing passes it
    count = 0.0;
    for (int64_t j = threadIdx.x; j < q.windows; j += MT) {           // a thread marks the windows it wrote itself
        const double l = lr_loudness(zw[j]);
        if (l > -70.0 && l > gate) count += 1.0; else zw[j] = -1.0;
    }
    const double m = block_sum(count, red);
    double lra = 0.0;
    if (m > 0.0) {
        const double k_lo = floor((m - 1.0) * 0.10 + 0.5), k_hi = floor((m - 1.0) * 0.95 + 0.5);
        unsigned long long p_lo = 0, p_hi = 0;
        for (int bit = 62; bit >= 0; --bit) {
            const unsigned long long c_lo = p_lo | (1ull << bit), c_hi = p_hi | (1ull << bit);
            double below_lo = 0.0, below_hi = 0.0;
            for (int64_t j = threadIdx.x; j < q.windows; j += MT) {
                const double z = zw[j];
                if (z < 0.0) continue;
                const unsigned long long b = (unsigned long long)__double_as_longlong(z);
                below_lo += b < c_lo ? 1.0 : 0.0;
                below_hi += b < c_hi ? 1.0 : 0.0;
            }
            below_lo = block_sum(below_lo, red);
            below_hi = block_sum(below_hi, red);
            if (below_lo <= k_lo) p_lo = c_lo;
            if (below_hi <= k_hi) p_hi = c_hi;
        }
        lra = lr_loudness(__longlong_as_double((long long)p_hi)) - lr_loudness(__longlong_as_double((long long)p_lo));
    }
    if (threadIdx.x == 0) {
        out[0] = lra;
        out[1] = blocks > 0 ? lr_loudness(z_m) : -INFINITY;
        out[2] = q.windows > 0 ? lr_loudness(z_st) : -INFINITY;
        out[3] = m;
    }
}

static int64_t lr_bytes(int64_t total_hops) { return (int64_t)align256((size_t)std::max<int64_t>(total_hops, 1) * 2 * sizeof(double)); }

extern "C" int64_t sos_loudness_range_workspace_bytes(const int64_t* table_host, int nfiles) {
    const char* who = "sos_loudness_range_workspace_bytes";
    if (!ragged_clips_ok(table_host, nfiles)) {
        sos_set_error("%s: bad args (1 .. 65535 files, got %d)", who, nfiles);
        return -1;
    }
    int64_t hops = 0;                                                // total chunks / split of the measurement, whatever its split
    for (int f = 0; f < nfiles; ++f) {
        const int64_t* te = table_host + (int64_t)f * LD_COLS;
        const int64_t ch = te[2], frames = te[3], h = te[5];
        if (ch < 1 || ch > LD_MAX_CHANNELS || frames < 0 || h < 1 || h > LD_MAX_HOP ||
            frames / h + (frames % h != 0) > (INT64_MAX / 64 - hops) / ch) {
            sos_set_error("%s: file %d (%lld channels, %lld frames, hop %lld) has channels outside 1 .. 64, a hop outside 1 .. 2^31 "
                          "or a length that is negative or too large", who, f, (long long)ch, (long long)frames, (long long)h);
            return -1;
        }
        hops += (frames / h + (frames % h != 0)) * ch;
    }
    return lr_bytes(hops);
}

extern "C" int sos_loudness_range_batch_f64(const int64_t* table, const int64_t* table_host, int nfiles, const double* weights, int split,
                                            const void* work, int64_t work_bytes, void* range_work, int64_t range_work_bytes,
                                            double* out, sos_stream_t stream) {
    const char* who = "sos_loudness_range_batch_f64";
    LdTotals t;
    const int rc = ld_args(who, !table || !table_host || !weights || !work || !range_work || !out, table_host, nfiles, split, true, &t);
    if (rc != SOS_OK) return rc;
    const int64_t need = (int64_t)align256((size_t)std::max<int64_t>(t.chunks, 1) * LD_WORK * sizeof(double));
    if (work_bytes < need || range_work_bytes < lr_bytes(t.chunks / split)) {
        sos_set_error("%s: the work buffers hold %lld and %lld bytes, %lld chunks need %lld and %lld", who, (long long)work_bytes,
                      (long long)range_work_bytes, (long long)t.chunks, (long long)need, (long long)lr_bytes(t.chunks / split));
        return SOS_ENOSPC;
    }
    hipStream_t st = (hipStream_t)stream;
    int64_t longest = 0;
    for (int f = 0; f < nfiles; ++f) longest = std::max(longest, table_host[(int64_t)f * LD_COLS + 3] / table_host[(int64_t)f * LD_COLS + 5]);
    hipLaunchKernelGGL(range_hops_kernel, dim3(ragged_grid(longest, MT, LD_MAX_GRID), (unsigned)nfiles), dim3(MT), 0, st, table, weights,
                       split, t.in, t.ch, t.chunks, (const double*)work, (double*)range_work);
    hipLaunchKernelGGL(range_gate_kernel, dim3((unsigned)nfiles), dim3(MT), 0, st, table, split, t.in, t.ch, t.chunks,
                       (double*)range_work, out);
    return sos_check_launch(who);
}
