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
// (SOS_EINVAL, naming the file), the kernels skip a row of the DEVICE table that fails the same rule.
#include "ragged.h"
#include <math.h>

#define LD_COLS 8                       // int64 per file: the encode row {first plane sample, plane length, channels, frames, -},
                                        // then {hop h, first channel weight, first chunk of the work arrays}
#define LD_WAVE 64                      // threads per workgroup of the chunk kernels: 64 consecutive chunks of one plane
#define LD_TILE 32                      // samples per chunk staged at a time
#define LD_MAX_CHANNELS 64
#define LD_MAX_SPLIT 64
#define LD_MAX_HOP ((int64_t)1 << 31)
#define LD_MAX_GRID 4096
#define LD_CARRY 8                      // chunk states the carry fetches ahead of its recurrence
#define LD_WORK 6                       // f64 arrays of the work buffer, one entry per chunk: state[4], energy, peak
#define LD_GAIN_THREADS 256
#define LD_GAIN_MAX_GRID 1024

__host__ __device__ static inline int64_t ld_min(int64_t a, int64_t b) { return a < b ? a : b; }

struct LdRow { int64_t first, avail, ch, frames, h, woff, qoff, nq; };         // nq: chunks per plane (the last hop may be partial)

// the plane side of a row, as pcm_io.hip holds it: `ch` planes of `avail` samples from `first` lie inside `total`
__host__ __device__ static inline bool ld_planes_inside(int64_t first, int64_t avail, int64_t ch, int64_t total) {
    return ch >= 1 && ch <= LD_MAX_CHANNELS && avail >= 0 && avail <= total / ch && ragged_clip_inside(first, avail * ch, total);
}

// the whole rule for a row of the measurement: planes, hop, weights and chunks inside the four totals
__host__ __device__ static inline bool ld_row(const int64_t* te, int split, int64_t total_in, int64_t total_ch, int64_t total_chunks,
                                              LdRow* r) {
    *r = {te[0], te[1], te[2], te[3], te[5], te[6], te[7], 0};
    if (!ld_planes_inside(r->first, r->avail, r->ch, total_in) || r->frames < 0 || r->h < split || r->h > LD_MAX_HOP) return false;
    const int64_t nh = r->frames / r->h + (r->frames % r->h != 0);
    if (nh > total_chunks / (split * r->ch)) return false;
    r->nq = nh * split;
    return ragged_clip_inside(r->woff, r->ch, total_ch) && ragged_clip_inside(r->qoff, r->nq * r->ch, total_chunks);
}

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

// Host: sums the table into the totals the kernels hold every device row to; nfiles, or the first row it cannot accept.
struct LdTotals { int64_t in = 0, ch = 0, chunks = 0, units = 0, longest = 0; };
static int ld_check_rows(const int64_t* table, int nfiles, int split, bool measure, LdTotals* t, const char** why) {
    for (int f = 0; f < nfiles; ++f) {
        const int64_t* te = table + (int64_t)f * LD_COLS;
        const int64_t avail = te[1], ch = te[2], frames = te[3], h = te[5];
        if (ch < 1 || ch > LD_MAX_CHANNELS) { *why = "channels outside 1 .. 64"; return f; }
        if (avail < 0 || avail > (INT64_MAX / 8 - t->in) / ch || frames < 0 || frames > INT64_MAX / 8 / ch) {
            *why = "a length that is negative or too large";
            return f;
        }
        t->in += avail * ch;
        t->ch += ch;
        t->longest = std::max(t->longest, std::min(avail, frames));
        if (!measure) continue;
        if (h < 1 || h > LD_MAX_HOP) { *why = "a hop outside 1 .. 2^31 samples"; return f; }
        if (h < split) { *why = "a hop shorter than the chunks per hop"; return f; }
        const int64_t nq = (frames / h + (frames % h != 0)) * split;
        if (nq > (INT64_MAX / 64 - t->chunks) / ch) { *why = "a length that is negative or too large"; return f; }
        t->chunks += nq * ch;
        t->units = std::max(t->units, (nq + LD_WAVE - 1) / LD_WAVE * ch);
    }
    for (int f = 0; f < nfiles; ++f) {
        const int64_t* te = table + (int64_t)f * LD_COLS;
        LdRow r;
        if (measure ? !ld_row(te, split, t->in, t->ch, t->chunks, &r) : !ld_planes_inside(te[0], te[1], te[2], t->in)) {
            *why = "a span outside the totals of the table";
            return f;
        }
    }
    return nfiles;
}

static int ld_args(const char* who, bool null, const int64_t* table_host, int nfiles, int split, bool measure, LdTotals* t) {
    if (null) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (!ragged_clips_ok(table_host, nfiles)) {
        sos_set_error("%s: bad args (1 .. 65535 files, got %d)", who, nfiles);
        return SOS_EINVAL;
    }
    if (measure && (split < 1 || split > LD_MAX_SPLIT)) {
        sos_set_error("%s: bad args (1 .. %d chunks per hop, got %d)", who, LD_MAX_SPLIT, split);
        return SOS_EINVAL;
    }
    const char* why = "";
    const int bad = ld_check_rows(table_host, nfiles, split, measure, t, &why);
    if (bad < nfiles) {
        const int64_t* te = table_host + (int64_t)bad * LD_COLS;
        sos_set_error("%s: file %d (plane sample %lld, %lld available, %lld channels, %lld frames, hop %lld, weight %lld, chunk "
                      "%lld) has %s (%lld plane samples, %lld channels, %lld chunks)", who, bad, (long long)te[0], (long long)te[1],
                      (long long)te[2], (long long)te[3], (long long)te[5], (long long)te[6], (long long)te[7], why,
                      (long long)t->in, (long long)t->ch, (long long)t->chunks);
        return SOS_EINVAL;
    }
    return SOS_OK;
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
