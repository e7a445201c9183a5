// ragged_window.hip -- the two copies around "a long recording as a ragged batch of overlapping windows" (pipeline.denoise_long;
// the plan is pipeline.window_plan, its float64 restatement tests/window_reference.py), each in ONE launch whatever the number
// of windows:
//   window_stage_kernel    a buffer of `total` floats + {source offset, samples} per window -> one zero-filled row per window.
//                          Windows may overlap and may start on any sample.
//   window_stitch_kernel   one row per window -> the recordings' outputs back to back.  Window k of a recording owns its core
//                          [core start, core end) of the output and is the ONE writer of those samples: a bit-for-bit copy of
//                          its own row, except in the `context` samples next to an inner core boundary b, where it blends its
//                          row with the neighbour's over the zone [b - context, b + context):
//                              w = (p - (b - context) + 0.5) / (2 context),  out = (1 - w) earlier + w later      (f32)
//                          The neighbour is named by the row itself (its table index), so nothing is searched; no atomics.
// Pure streaming, shaped like ragged_io.hip: a thread handles four consecutive samples, one 16-byte access where the address
// allows it and scalar accesses otherwise; which of the two is taken changes no value, so a recording's output has the same bits
// alone, in any batch, at any offset and with the table in any order.
//   window_stitch_planes_kernel   window_stitch_kernel for up to eight signals of the SAME plan (rows [planes][n_rows][stride]) in
//                          one launch: the four signals of denoise_long(signals=True) and of the windowed hand-off.  Each plane
//                          holds the bits window_stitch_kernel gives for it alone (window_quad is the one statement of the
//                          arithmetic); sample p of plane q of recording r goes to out[base_r + q pitch_r + p], {base, pitch} per
//                          recording, so one launch writes plane-major or file-major, where the download wants the samples.
// Two more for the detector half of the chain and the `bits=` path (pipeline.detect_long / denoise_long):
//   window_frames_stitch_kernel   one row of frame logits per window -> ONE logit stream per recording.  The windows' frame grids
//                          do not line up with the recording's (a frame is rho = sr / fps samples, windows start on samples), so
//                          frame i of the recording is placed by its centre p = (i + 0.5) rho: the window whose core holds p owns
//                          it and gives the frame of its own grid that holds p, j = clamp(floor((i + 0.5) - start / rho), 0,
//                          frames - 1); within `context` samples of an inner core boundary the two neighbours' frames are blended
//                          with w = (p - (b - context)) / (2 context) (float64, rounded once to f32; blend in f32).  float64
//                          restatement: tests/frames_reference.py.  One thread and one writer per output frame.
//   window_stage_masked_kernel    window_stage_kernel plus the mask rule (mask_rule.h) in the RECORDING's coordinates: the windows'
//                          wave rows and their masked rows x * mask, mask = mask_sample(bits of the recording, its frames, its
//                          ratio, its samples, window start + j): slices of what sos_ragged_stage_f32 makes at full length, bit
//                          for bit, with nothing of full length written.
//   window_frames_link_kernel     window_frames_stitch_kernel with a link table: the stitched logits of the recordings of a GROUP
//                          (the channels of a file) reduced in member order -- any: fmaxf, mean: a sequential f32 sum and one
//                          divide -- and thresholded (mask_rule.h: frame_decision), ONE logit and ONE decision stream per group
//                          in one launch.  stitched_frame is the one statement of the stitch both kernels call; numpy
//                          restatement of the reduction and the decision: tests/link_reference.py.
// Bounds: the rule of ragged.h -- the host refuses a table entry that leaves what it sized from table_host (SOS_EINVAL), the
// kernels skip an entry of the DEVICE table that fails the same test (window_stage_ok / window_stitch_why / frames_rec_ok /
// frames_win_ok / window_masked_ok below).
#include "ragged.h"
#include "mask_rule.h"
#include <cmath>
#include <utility>
#include <vector>

#define RW_THREADS 256
#define RW_MAX_GRID 1024                // workgroups along a row (they stride over what the grid does not cover)
#define RW_STITCH_QUADS 4               // quads per thread the stitch grid is sized for
#define RW_MAX_PLANES 8                 // signals one planes stitch takes
#define RW_COLS 10                      // int64 per window, the row of pipeline.window_plan
#define RW_MAX_CONTEXT ((int64_t)1 << 22)   // 2 context + 0.5 is exact in f32
#define RW_REC_COLS 4                   // int64 per recording of the frame stitch: frame offset in the output, frames, first window, windows
#define RW_MAX_FRAMES ((int64_t)1 << 31)    // frames of a recording and
#define RW_MAX_RATIO 1073741824.0           // samples per frame (2^30): a frame centre (i + 0.5) rho stays inside int64

// One window.  rec: the recording (not read here); off: first source sample in the staged buffer; n: samples; out: where the
// window's first output sample lies in the stitched buffer; cs, ce, start: core start, core end and the window's first sample
// in the recording's own coordinates; row: the window's row in `rows` of the stitch; prev, next: table indices of the windows
// before and after it in the same recording, -1 at the recording's ends.
struct WindowRow { int64_t rec, off, n, out, cs, ce, start, row, prev, next; };
__host__ __device__ static inline WindowRow window_row(const int64_t* table, int64_t w) {
    const int64_t* te = table + w * RW_COLS;
    return {te[0], te[1], te[2], te[3], te[4], te[5], te[6], te[7], te[8], te[9]};
}

__host__ __device__ static inline bool window_stage_ok(const WindowRow& e, int64_t stride, int64_t total) {
    return e.n <= stride && ragged_clip_inside(e.off, e.n, total);
}

// Why window w of a stitch table cannot be followed (0: it can).  Every comparison is between values already known to lie in
// [0, INT64_MAX / 8], so no sum overflows.
enum { RW_OK = 0, RW_ROW, RW_SAMPLES, RW_CORE, RW_OUTPUT, RW_NEIGHBOUR, RW_CONTEXT };
__host__ __device__ static inline bool window_small(int64_t v) { return v >= 0 && v <= INT64_MAX / 8; }
__host__ __device__ static inline int window_stitch_why(const int64_t* table, int64_t w, int64_t nwin, int64_t n_rows, int64_t stride,
                                                        int64_t context, int64_t total_out, bool neighbours = true) {
    const WindowRow e = window_row(table, w);
    if (e.row < 0 || e.row >= n_rows) return RW_ROW;
    if (e.n < 0 || e.n > stride) return RW_SAMPLES;
    // the core lies inside the window's own samples
    if (!window_small(e.start) || !window_small(e.cs) || !window_small(e.ce) || e.start > e.cs || e.cs > e.ce || e.ce - e.start > e.n)
        return RW_CORE;
    const int64_t len = e.ce - e.cs;
    if (!window_small(e.out) || e.out > total_out || !ragged_clip_inside(e.out + (e.cs - e.start), len, total_out)) return RW_OUTPUT;
    if (context == 0 || !neighbours) return RW_OK;               // a plain cut: no neighbour is read
    const int zones = (e.prev >= 0) + (e.next >= 0);
    if (zones && (context >= e.n || zones * context > len)) return RW_CONTEXT;
    for (int side = 0; side < 2; ++side) {
        const int64_t o = side ? e.next : e.prev;
        if (o < 0) continue;
        if (o >= nwin || o == w) return RW_NEIGHBOUR;
        const WindowRow q = window_row(table, o);
        if (q.row < 0 || q.row >= n_rows || q.n < 0 || q.n > stride || !window_small(q.start) || !window_small(q.out)) return RW_NEIGHBOUR;
        if (q.out - q.start != e.out - e.start) return RW_NEIGHBOUR;                     // another recording's coordinates
        if (context >= q.n) return RW_CONTEXT;
        // the samples this window reads of the neighbour's row: [cs, cs + context) of the one before, [ce - context, ce) of the one after
        const int64_t lo = side ? e.ce - context : e.cs, hi = lo + context;
        if (q.start > lo || hi - q.start > q.n) return RW_NEIGHBOUR;
    }
    return RW_OK;
}

__global__ __launch_bounds__(RW_THREADS) void window_stage_kernel(const float* __restrict__ x, int64_t total,
                                                                 const int64_t* __restrict__ table, int64_t stride,
                                                                 float* __restrict__ rows) {
    const int64_t w = blockIdx.y;
    const WindowRow e = window_row(table, w);
    if (!window_stage_ok(e, stride, total)) return;
    const float* src = x + e.off;
    float* dst = rows + w * stride;
    const int64_t n = e.n;
    const bool row_vec = (stride & 3) == 0 && ragged_aligned16(rows), src_vec = ragged_aligned16(src);
    for (int64_t j0 = ((int64_t)blockIdx.x * RW_THREADS + threadIdx.x) * 4; j0 < stride; j0 += (int64_t)gridDim.x * RW_THREADS * 4) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};                      // zero from the window's end to the stride
        ragged_load4(src, j0, n, j0 + 4 <= n && src_vec, v);
        ragged_store4(dst, j0, stride, row_vec, v);             // row_vec: the stride is a multiple of four, so j0 + 4 <= stride
    }
}

// v[k] = base[i0 + k] for the samples j0 + k of [jlo, jhi): one 16-byte load where all four are wanted and the address allows it
__device__ __forceinline__ void window_load4(const float* base, int64_t i0, int64_t j0, int64_t jlo, int64_t jhi, float (&v)[4]) {
    if (j0 >= jlo && j0 + 4 <= jhi && ragged_aligned16(base + i0)) {
        const ragged_f32x4 q = *(const ragged_f32x4*)(base + i0);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + k >= jlo && j0 + k < jhi) v[k] = base[i0 + k];
    }
}

// The zones of a core of `len` samples: sample j < head blends with the window before, j >= tail with the window after;
// before / after: the element of `rows` that holds sample cs of that neighbour's row.
struct WindowZones { int64_t head, tail, before, after; };
__device__ __forceinline__ WindowZones window_zones(const int64_t* table, const WindowRow& e, int64_t stride, int64_t context) {
    const int64_t len = e.ce - e.cs;
    WindowZones z = {context > 0 && e.prev >= 0 ? context : 0, context > 0 && e.next >= 0 ? len - context : len, 0, 0};
    if (z.head) {
        const WindowRow q = window_row(table, e.prev);
        z.before = q.row * stride + (e.cs - q.start);
    }
    if (z.tail < len) {
        const WindowRow q = window_row(table, e.next);
        z.after = q.row * stride + (e.cs - q.start);            // negative for a while: only j >= tail is read
    }
    return z;
}

// The quad j0 .. j0 + 3 of a core (element own + j of `rows` holds its sample j): v = the window's own samples, blended with
// the neighbour's inside the zones.  The ONE statement of the stitch's arithmetic: window_stitch_kernel and
// window_stitch_planes_kernel (rows = the plane's) both call it.
__device__ __forceinline__ void window_quad(const float* rows, int64_t own, const WindowZones& z, int64_t j0, int64_t len,
                                            int64_t context, float span, float (&v)[4]) {
    window_load4(rows, own + j0, j0, 0, len, v);
    if (j0 < z.head) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        window_load4(rows, z.before + j0, j0, 0, z.head, a);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + k < z.head) {
                const float wt = ((float)(j0 + k + context) + 0.5f) / span;
                v[k] = (1.f - wt) * a[k] + wt * v[k];
            }
    }
    if (j0 + 4 > z.tail) {
        float b[4] = {0.f, 0.f, 0.f, 0.f};
        window_load4(rows, z.after + j0, j0, z.tail, len, b);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + k >= z.tail && j0 + k < len) {
                const float wt = ((float)(j0 + k - z.tail) + 0.5f) / span;
                v[k] = (1.f - wt) * v[k] + wt * b[k];
            }
    }
}

__global__ __launch_bounds__(RW_THREADS) void window_stitch_kernel(const float* __restrict__ rows, int64_t n_rows, int64_t stride,
                                                                  const int64_t* __restrict__ table, int64_t nwin, int64_t context,
                                                                  int64_t total_out, float* __restrict__ out) {
    const int64_t w = blockIdx.y;
    if (window_stitch_why(table, w, nwin, n_rows, stride, context, total_out) != RW_OK) return;
    const WindowRow e = window_row(table, w);
    const int64_t len = e.ce - e.cs;                            // sample j of the core is sample cs + j of the recording
    const int64_t own = e.row * stride + (e.cs - e.start);      // ... and element own + j of `rows`
    float* dst = out + e.out + (e.cs - e.start);
    const bool dst_vec = ragged_aligned16(dst);
    const WindowZones z = window_zones(table, e, stride, context);
    const float span = (float)(2 * context);
    for (int64_t j0 = ((int64_t)blockIdx.x * RW_THREADS + threadIdx.x) * 4; j0 < len; j0 += (int64_t)gridDim.x * RW_THREADS * 4) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        window_quad(rows, own, z, j0, len, context, span, v);
        ragged_store4(dst, j0, len, j0 + 4 <= len && dst_vec, v);
    }
}

// Where a recording's planes go: sample p of plane q lies at out[base + q * pitch + p].
struct PlaneRec { int64_t base, pitch; };
__host__ __device__ static inline PlaneRec plane_rec(const int64_t* recs, int64_t r) { return {recs[2 * r], recs[2 * r + 1]}; }
// `extent` samples of every plane (the host: the recording's output length; the kernel: up to the window's core end) lie inside
// the out_total floats and inside their own plane.  planes <= 8 and every term <= INT64_MAX / 8: no sum overflows.
__host__ __device__ static inline bool planes_inside(const PlaneRec& d, int planes, int64_t extent, int64_t out_total) {
    if (!window_small(out_total) || d.base < 0 || d.base > out_total || extent < 0 || d.pitch < extent) return false;
    if (planes > 1 && d.pitch > out_total / (planes - 1)) return false;
    return ragged_clip_inside(d.base + (planes > 1 ? (planes - 1) * d.pitch : 0), extent, out_total);
}

#ifndef RW_PLANES_IN_GRID
#define RW_PLANES_IN_GRID 0             // 1: one grid.z slice per plane instead of the inner loop: 134 us against 81 us (EXPERIMENTS.md 3.16)
#endif

// window_stitch_kernel for `planes` signals of the same plan: the table decode, the zone tests and the weights are the
// window's, only the rows and the destination are the plane's.  A thread takes its quad through the planes gridDim.z apart.
__global__ __launch_bounds__(RW_THREADS) void window_stitch_planes_kernel(
    const float* __restrict__ rows, int planes, int64_t n_rows, int64_t stride, const int64_t* __restrict__ table, int64_t nwin,
    int64_t context, int64_t total_core, const int64_t* __restrict__ recs, int64_t nrec, int64_t out_total,
    float* __restrict__ out) {
    const int64_t w = blockIdx.y;
    if (window_stitch_why(table, w, nwin, n_rows, stride, context, total_core) != RW_OK) return;
    const WindowRow e = window_row(table, w);
    if (e.rec < 0 || e.rec >= nrec) return;
    const PlaneRec d = plane_rec(recs, e.rec);
    if (!planes_inside(d, planes, e.ce, out_total)) return;
    const int64_t len = e.ce - e.cs;
    const int64_t own = e.row * stride + (e.cs - e.start);
    const WindowZones z = window_zones(table, e, stride, context);
    if ((z.head && window_row(table, e.prev).rec != e.rec) || (z.tail < len && window_row(table, e.next).rec != e.rec)) return;
    const float span = (float)(2 * context);
    const int64_t plane = n_rows * stride;
    for (int64_t j0 = ((int64_t)blockIdx.x * RW_THREADS + threadIdx.x) * 4; j0 < len; j0 += (int64_t)gridDim.x * RW_THREADS * 4)
        for (int q = blockIdx.z; q < planes; q += gridDim.z) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            window_quad(rows + q * plane, own, z, j0, len, context, span, v);
            float* dst = out + d.base + q * d.pitch + e.cs;
            ragged_store4(dst, j0, len, j0 + 4 <= len && ragged_aligned16(dst), v);
        }
}

static bool window_args_ok(const char* who, const void* a, const void* b, const int64_t* table, const int64_t* table_host, int nwin,
                           int64_t stride) {
    if (!a || !b || !table || !table_host) { sos_set_error("%s: null pointer", who); return false; }
    if (nwin < 1 || nwin > RAGGED_MAX_CLIPS || stride < 1 || stride > INT64_MAX / 8 / RAGGED_MAX_CLIPS) {
        sos_set_error("%s: bad args (1 .. 65535 windows, got %d; stride %lld)", who, nwin, (long long)stride);
        return false;
    }
    return true;
}

extern "C" int sos_window_stage_f32(const float* x, int64_t total, const int64_t* table, const int64_t* table_host, int nwin,
                                    int64_t stride, float* rows, sos_stream_t stream) {
    if (!window_args_ok("sos_window_stage_f32", x, rows, table, table_host, nwin, stride)) return SOS_EINVAL;
    if (total < 0 || total > INT64_MAX / 8) {
        sos_set_error("sos_window_stage_f32: a buffer of %lld samples", (long long)total);
        return SOS_EINVAL;
    }
    for (int w = 0; w < nwin; ++w) {
        const WindowRow e = window_row(table_host, w);
        if (e.n > stride) {
            sos_set_error("sos_window_stage_f32: window %d has %lld samples (stride %lld)", w, (long long)e.n, (long long)stride);
            return SOS_EINVAL;
        }
        if (!window_stage_ok(e, stride, total)) {
            sos_set_error("sos_window_stage_f32: window %d (samples %lld + %lld) lies outside the %lld samples of the buffer", w,
                          (long long)e.off, (long long)e.n, (long long)total);
            return SOS_EINVAL;
        }
    }
    const dim3 grid(ragged_grid((stride + 3) / 4, RW_THREADS, RW_MAX_GRID), (unsigned)nwin);
    hipLaunchKernelGGL(window_stage_kernel, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, x, total, table, stride, rows);
    return sos_check_launch("sos_window_stage_f32");
}

// What both stitches refuse of a plan, before any launch: false with the error set (it names the window), else the summed
// output length the cores tile and the longest core.
static bool window_stitch_plan_ok(const char* who, const int64_t* table_host, int nwin, int64_t n_rows, int64_t stride,
                                  int64_t context, int64_t* total_out_p, int64_t* longest_p) {
    if (n_rows < 1 || n_rows > INT64_MAX / 8 / stride || context < 0 || context > RW_MAX_CONTEXT) {
        sos_set_error("%s: bad args (%lld rows of %lld; context %lld, 0 .. %lld)", who, (long long)n_rows, (long long)stride,
                      (long long)context, (long long)RW_MAX_CONTEXT);
        return false;
    }
    // the summed output length: the cores tile the recordings' outputs
    int64_t total_out = 0, longest = 0;
    for (int w = 0; w < nwin; ++w) {
        const WindowRow e = window_row(table_host, w);
        if (!window_small(e.cs) || !window_small(e.ce) || e.cs > e.ce || e.ce - e.cs > INT64_MAX / 8 - total_out) {
            sos_set_error("%s: window %d has the core %lld .. %lld", who, w, (long long)e.cs, (long long)e.ce);
            return false;
        }
        total_out += e.ce - e.cs;
        longest = std::max(longest, e.ce - e.cs);
    }
    for (int pass = 0; pass < 2 * nwin; ++pass) {              // every window by itself first: the message names the wrong one
        const int w = pass % nwin;
        const int why = window_stitch_why(table_host, w, nwin, n_rows, stride, context, total_out, pass >= nwin);
        if (why == RW_OK) continue;
        const WindowRow e = window_row(table_host, w);
        static const char* const reason[] = {"", "names a row outside the rows", "has more samples than the stride",
                                             "has a core outside its own samples", "writes outside the summed output length",
                                             "names a neighbour that is no window of its recording or does not cover the overlap",
                                             "blends over a context that is not less than the window, or more than its core holds"};
        sos_set_error("%s: window %d %s (row %lld of %lld, samples %lld, stride %lld, start %lld, core %lld .. "
                      "%lld, output %lld of %lld, neighbours %lld and %lld, context %lld)", who, w, reason[why], (long long)e.row,
                      (long long)n_rows, (long long)e.n, (long long)stride, (long long)e.start, (long long)e.cs, (long long)e.ce,
                      (long long)e.out, (long long)total_out, (long long)e.prev, (long long)e.next, (long long)context);
        return false;
    }
    *total_out_p = total_out;
    *longest_p = longest;
    return true;
}

extern "C" int sos_window_stitch_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table,
                                     const int64_t* table_host, int nwin, int64_t context, float* out, sos_stream_t stream) {
    if (!window_args_ok("sos_window_stitch_f32", rows, out, table, table_host, nwin, stride)) return SOS_EINVAL;
    int64_t total_out = 0, longest = 0;
    if (!window_stitch_plan_ok("sos_window_stitch_f32", table_host, nwin, n_rows, stride, context, &total_out, &longest)) return SOS_EINVAL;
    // four quads per thread: a workgroup reads its row and both neighbours' before its first sample, which few samples do not repay
    const dim3 grid(ragged_grid((longest + 3) / 4, RW_THREADS * RW_STITCH_QUADS, RW_MAX_GRID), (unsigned)nwin);
    hipLaunchKernelGGL(window_stitch_kernel, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, rows, n_rows, stride, table,
                       (int64_t)nwin, context, total_out, out);
    return sos_check_launch("sos_window_stitch_f32");
}

extern "C" int sos_window_stitch_planes_f32(const float* rows, int planes, int64_t n_rows, int64_t stride, const int64_t* table,
                                            const int64_t* table_host, int nwin, int64_t context, const int64_t* recs,
                                            const int64_t* recs_host, int nrec, int64_t out_total, float* out,
                                            sos_stream_t stream) {
    const char* who = "sos_window_stitch_planes_f32";
    if (!window_args_ok(who, rows, out, table, table_host, nwin, stride)) return SOS_EINVAL;
    if (!recs || !recs_host) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (planes < 1 || planes > RW_MAX_PLANES || nrec < 1 || nrec > RAGGED_MAX_CLIPS || !window_small(out_total)) {
        sos_set_error("%s: bad args (1 .. %d planes, got %d; 1 .. 65535 recordings, got %d; an output of %lld floats)", who,
                      RW_MAX_PLANES, planes, nrec, (long long)out_total);
        return SOS_EINVAL;
    }
    int64_t total_core = 0, longest = 0;
    if (!window_stitch_plan_ok(who, table_host, nwin, n_rows, stride, context, &total_core, &longest)) return SOS_EINVAL;
    if (n_rows > INT64_MAX / 8 / stride / planes) {
        sos_set_error("%s: bad args (%d planes of %lld rows of %lld)", who, planes, (long long)n_rows, (long long)stride);
        return SOS_EINVAL;
    }
    // a recording's output length: the sum of its cores
    std::vector<int64_t> len(nrec, 0);
    for (int w = 0; w < nwin; ++w) {
        const WindowRow e = window_row(table_host, w);
        if (e.rec < 0 || e.rec >= nrec) {
            sos_set_error("%s: window %d names recording %lld of %d", who, w, (long long)e.rec, nrec);
            return SOS_EINVAL;
        }
        len[e.rec] += e.ce - e.cs;
    }
    for (int w = 0; w < nwin; ++w) {
        const WindowRow e = window_row(table_host, w);
        if (e.ce > len[e.rec]) {
            sos_set_error("%s: window %d has the core %lld .. %lld, outside the %lld output samples of recording %lld (the sum of "
                          "its cores)", who, w, (long long)e.cs, (long long)e.ce, (long long)len[e.rec], (long long)e.rec);
            return SOS_EINVAL;
        }
        for (int side = 0; side < 2 && context > 0; ++side) {
            const int64_t o = side ? e.next : e.prev;
            if (o >= 0 && window_row(table_host, o).rec != e.rec) {
                sos_set_error("%s: window %d of recording %lld has the neighbour %lld, a window of recording %lld", who, w,
                              (long long)e.rec, (long long)o, (long long)window_row(table_host, o).rec);
                return SOS_EINVAL;
            }
        }
    }
    std::vector<std::pair<int64_t, int>> seg;                   // {start, recording * planes + plane} of the segments that hold samples
    for (int r = 0; r < nrec; ++r) {
        const PlaneRec d = plane_rec(recs_host, r);
        if (d.pitch < len[r]) {
            sos_set_error("%s: recording %d has the pitch %lld, less than its %lld output samples", who, r, (long long)d.pitch,
                          (long long)len[r]);
            return SOS_EINVAL;
        }
        if (!planes_inside(d, planes, len[r], out_total)) {
            sos_set_error("%s: recording %d (base %lld, pitch %lld, %lld samples in each of %d planes) lies outside the %lld "
                          "floats of the output", who, r, (long long)d.base, (long long)d.pitch, (long long)len[r], planes,
                          (long long)out_total);
            return SOS_EINVAL;
        }
        for (int q = 0; q < planes && len[r] > 0; ++q) seg.push_back({d.base + q * d.pitch, r * planes + q});
    }
    std::sort(seg.begin(), seg.end());
    for (size_t i = 1; i < seg.size(); ++i) {
        const int a = seg[i - 1].second, b = seg[i].second;
        if (seg[i].first < seg[i - 1].first + len[a / planes]) {
            sos_set_error("%s: plane %d of recording %d (%lld + %lld) and plane %d of recording %d (from %lld) overlap in the "
                          "output", who, a % planes, a / planes, (long long)seg[i - 1].first, (long long)len[a / planes],
                          b % planes, b / planes, (long long)seg[i].first);
            return SOS_EINVAL;
        }
    }
    const dim3 grid(ragged_grid((longest + 3) / 4, RW_THREADS * RW_STITCH_QUADS, RW_MAX_GRID), (unsigned)nwin,
                    RW_PLANES_IN_GRID ? (unsigned)planes : 1u);
    hipLaunchKernelGGL(window_stitch_planes_kernel, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, rows, planes, n_rows, stride,
                       table, (int64_t)nwin, context, total_core, recs, (int64_t)nrec, out_total, out);
    return sos_check_launch(who);
}

// ---- one logit stream per recording out of the windows' frame logits

struct FrameRec { int64_t foff, F, first, K; };            // frame offset in the output, frames, first window (table index), windows
__host__ __device__ static inline FrameRec frame_rec(const int64_t* recs, int64_t r) {
    const int64_t* te = recs + r * RW_REC_COLS;
    return {te[0], te[1], te[2], te[3]};
}
// a recording can be followed: its frames lie inside the summed output, its windows inside the table, its ratio places every
// frame centre inside int64 (a NaN fails rho > 0)
__host__ __device__ static inline bool frames_rec_windows_ok(const FrameRec& r, double rho, int64_t nwin) {
    return r.F >= 0 && r.F <= RW_MAX_FRAMES && r.first >= 0 && r.K >= 1 && r.K <= nwin && r.first <= nwin - r.K && rho > 0.0 &&
           rho <= RW_MAX_RATIO;
}
__host__ __device__ static inline bool frames_rec_ok(const FrameRec& r, double rho, int64_t nwin, int64_t total_frames) {
    return ragged_clip_inside(r.foff, r.F, total_frames) && frames_rec_windows_ok(r, rho, nwin);
}
// a window can be read: its row exists and holds its `frames` logits
__host__ __device__ static inline bool frames_win_ok(const WindowRow& e, int64_t frames, int64_t n_rows, int64_t stride) {
    return e.row >= 0 && e.row < n_rows && frames >= 1 && frames <= stride && window_small(e.start) && window_small(e.cs) &&
           window_small(e.ce) && e.cs <= e.ce;
}

// Frame of a window (first sample `start` of the recording, `frames` frames) that holds the centre of the recording's frame
// i, c = i + 0.5: clamp(floor(c - start / rho), 0, frames - 1).  One rounded divide, one rounded subtract (un-fused).
__device__ __forceinline__ int64_t frame_in_window(double c, int64_t start, double rho, int64_t frames) {
    const double j = floor(__dadd_rn(c, -__ddiv_rn((double)start, rho)));
    return j < 0.0 ? 0 : j > (double)(frames - 1) ? frames - 1 : (int64_t)j;
}

// The stitched logit of frame i of ONE recording (`rec`, rho samples per frame; span = 2 context): the ONE statement of the
// frame stitch's arithmetic, window_frames_stitch_kernel and window_frames_link_kernel both call it.  false: a window it needs
// fails frames_win_ok, and the frame is left alone.
__device__ __forceinline__ bool stitched_frame(const float* __restrict__ rows, int64_t n_rows, int64_t stride,
                                               const int64_t* __restrict__ table, const int64_t* __restrict__ frames,
                                               const FrameRec& rec, double rho, int64_t core, int64_t context, double span,
                                               int64_t i, float* out) {
    const double c = (double)i + 0.5;                           // exact
    const double p = __dmul_rn(c, rho);                         // the frame's centre, in samples of the recording
    const int64_t own = (int64_t)p / core, k = own < rec.K - 1 ? own : rec.K - 1;      // frames past the last core belong to the last window
    const int64_t w = rec.first + k;
    const WindowRow e = window_row(table, w);
    const int64_t fe = frames[w];
    if (!frames_win_ok(e, fe, n_rows, stride)) return false;
    float v = rows[e.row * stride + frame_in_window(c, e.start, rho, fe)];
    if (context > 0) {
        // core >= 2 context: at most one of the two zones holds p
        const int side = k > 0 && p < (double)(e.cs + context) ? -1 : k < rec.K - 1 && p >= (double)(e.ce - context) ? 1 : 0;
        if (side) {
            const WindowRow q = window_row(table, w + side);
            const int64_t fq = frames[w + side];
            if (!frames_win_ok(q, fq, n_rows, stride)) return false;
            const float u = rows[q.row * stride + frame_in_window(c, q.start, rho, fq)];
            const double b = (double)((side < 0 ? e.cs : e.ce) - context);
            const float wt = (float)__ddiv_rn(__dadd_rn(p, -b), span);   // float64, rounded once
            v = side < 0 ? (1.f - wt) * u + wt * v : (1.f - wt) * v + wt * u;
        }
    }
    *out = v;
    return true;
}

__global__ __launch_bounds__(RW_THREADS) void window_frames_stitch_kernel(
    const float* __restrict__ rows, int64_t n_rows, int64_t stride, const int64_t* __restrict__ table,
    const int64_t* __restrict__ frames, int64_t nwin, const int64_t* __restrict__ recs, const double* __restrict__ ratios,
    int64_t core, int64_t context, int64_t total_frames, float* __restrict__ out) {
    const int64_t r = blockIdx.y;
    const FrameRec rec = frame_rec(recs, r);
    const double rho = ratios[r];
    if (core < 1 || !frames_rec_ok(rec, rho, nwin, total_frames)) return;
    float* dst = out + rec.foff;
    const double span = (double)(2 * context);
    for (int64_t i = (int64_t)blockIdx.x * RW_THREADS + threadIdx.x; i < rec.F; i += (int64_t)gridDim.x * RW_THREADS) {
        float v;
        if (stitched_frame(rows, n_rows, stride, table, frames, rec, rho, core, context, span, i, &v)) dst[i] = v;
    }
}

// ---- one logit and one decision stream per GROUP of linked recordings (the channels of a file)

#define RW_LINK_COLS 4                  // int64 per group: frame offset in the outputs, frames, first index into `members`, members
struct LinkRow { int64_t foff, F, first, count; };
__host__ __device__ static inline LinkRow link_row(const int64_t* links, int64_t g) {
    const int64_t* te = links + g * RW_LINK_COLS;
    return {te[0], te[1], te[2], te[3]};
}
// a group can be followed: its stream lies inside the summed output, its members inside `members`
__host__ __device__ static inline bool link_ok(const LinkRow& lk, int64_t nmem, int64_t total_frames) {
    return ragged_clip_inside(lk.foff, lk.F, total_frames) && lk.count >= 1 && ragged_clip_inside(lk.first, lk.count, nmem);
}

// window_frames_stitch_kernel with a link table: the stitched logits of a group's members reduced in member order (mode 0:
// fmaxf, mode 1: a sequential f32 sum and one f32 divide by the member count) and thresholded (mask_rule.h), one thread and
// one writer per frame of the group.  The members' own frame offsets (column 0 of `recs`) are not read.
__global__ __launch_bounds__(RW_THREADS) void window_frames_link_kernel(
    const float* __restrict__ rows, int64_t n_rows, int64_t stride, const int64_t* __restrict__ table,
    const int64_t* __restrict__ frames, int64_t nwin, const int64_t* __restrict__ recs, const double* __restrict__ ratios,
    int64_t nrec, const int64_t* __restrict__ links, const int64_t* __restrict__ members, int64_t nmem, int64_t core,
    int64_t context, int mode, float thr, int64_t total_frames, float* __restrict__ out_logits, uint8_t* __restrict__ out_bits) {
    const LinkRow lk = link_row(links, blockIdx.y);
    if (core < 1 || !link_ok(lk, nmem, total_frames)) return;
    const int64_t* mem = members + lk.first;
    for (int64_t m = 0; m < lk.count; ++m) {                    // every member can be followed, or the group gets no work
        const int64_t r = mem[m];
        if (r < 0 || r >= nrec) return;
        const FrameRec rec = frame_rec(recs, r);
        if (rec.F != lk.F || !frames_rec_windows_ok(rec, ratios[r], nwin)) return;
    }
    const double span = (double)(2 * context);
    for (int64_t i = (int64_t)blockIdx.x * RW_THREADS + threadIdx.x; i < lk.F; i += (int64_t)gridDim.x * RW_THREADS) {
        float acc = 0.f;
        bool ok = true;
        for (int64_t m = 0; m < lk.count && ok; ++m) {
            const int64_t r = mem[m];
            float v = 0.f;
            ok = stitched_frame(rows, n_rows, stride, table, frames, frame_rec(recs, r), ratios[r], core, context, span, i, &v);
            acc = m == 0 ? v : mode == 0 ? fmaxf(acc, v) : acc + v;
        }
        if (!ok) continue;
        if (mode == 1) acc = acc / (float)lk.count;
        out_logits[lk.foff + i] = acc;
        out_bits[lk.foff + i] = frame_decision(acc, thr);
    }
}

// What both frame entries refuse of their arguments, before any table is read: false with the error set.
static bool frames_args_ok(const char* who, const float* rows, const void* out, const int64_t* table, const int64_t* table_host,
                           const int64_t* frames, const int64_t* frames_host, int nwin, const int64_t* recs,
                           const int64_t* recs_host, const double* ratios, const double* ratios_host, int nrec, int64_t n_rows,
                           int64_t stride, int64_t core, int64_t context) {
    if (!window_args_ok(who, rows, out, table, table_host, nwin, stride)) return false;
    if (!frames || !frames_host || !recs || !recs_host || !ratios || !ratios_host) { sos_set_error("%s: null pointer", who); return false; }
    if (nrec < 1 || nrec > RAGGED_MAX_CLIPS || n_rows < 1 || n_rows > INT64_MAX / 8 / stride || core < 1 || context < 0 ||
        context > RW_MAX_CONTEXT || core < 2 * context) {
        sos_set_error("%s: bad args (1 .. 65535 recordings, got %d; %lld rows of %lld; core %lld >= 1 and >= twice the context "
                      "%lld, 0 .. %lld)", who, nrec, (long long)n_rows, (long long)stride, (long long)core, (long long)context,
                      (long long)RW_MAX_CONTEXT);
        return false;
    }
    return true;
}

// Every window of recording r can be read: false with the error set, which names the window.
static bool frames_windows_ok(const char* who, int r, const FrameRec& rec, const int64_t* table_host, const int64_t* frames_host,
                              int64_t n_rows, int64_t stride) {
    for (int64_t w = rec.first; w < rec.first + rec.K; ++w) {
        const WindowRow e = window_row(table_host, w);
        if (!frames_win_ok(e, frames_host[w], n_rows, stride)) {
            sos_set_error("%s: window %lld of recording %d names a row outside the rows, or frames outside the stride (row "
                          "%lld of %lld, frames %lld, stride %lld, start %lld, core %lld .. %lld)", who, (long long)w, r,
                          (long long)e.row, (long long)n_rows, (long long)frames_host[w], (long long)stride,
                          (long long)e.start, (long long)e.cs, (long long)e.ce);
            return false;
        }
    }
    return true;
}

extern "C" int sos_window_frames_stitch_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table,
                                            const int64_t* table_host, const int64_t* frames, const int64_t* frames_host, int nwin,
                                            const int64_t* recs, const int64_t* recs_host, const double* ratios,
                                            const double* ratios_host, int nrec, int64_t core, int64_t context, float* out,
                                            sos_stream_t stream) {
    const char* who = "sos_window_frames_stitch_f32";
    if (!frames_args_ok(who, rows, out, table, table_host, frames, frames_host, nwin, recs, recs_host, ratios, ratios_host, nrec,
                        n_rows, stride, core, context))
        return SOS_EINVAL;
    RaggedSum nf;
    int bad = ragged_sum_column(recs_host, nrec, RW_REC_COLS, 1, 0, RW_MAX_FRAMES, &nf);
    if (bad < nrec) {
        sos_set_error("%s: recording %d has %lld frames (0 .. %lld)", who, bad, (long long)frame_rec(recs_host, bad).F,
                      (long long)RW_MAX_FRAMES);
        return SOS_EINVAL;
    }
    for (int r = 0; r < nrec; ++r) {
        const FrameRec rec = frame_rec(recs_host, r);
        if (!frames_rec_ok(rec, ratios_host[r], nwin, nf.total)) {
            sos_set_error("%s: recording %d (frames %lld + %lld of %lld, windows %lld + %lld of %d, %g samples per frame) lies "
                          "outside the output or the table, or has a ratio outside (0, 2^30]", who, r, (long long)rec.foff,
                          (long long)rec.F, (long long)nf.total, (long long)rec.first, (long long)rec.K, nwin, ratios_host[r]);
            return SOS_EINVAL;
        }
        if (!frames_windows_ok(who, r, rec, table_host, frames_host, n_rows, stride)) return SOS_EINVAL;
    }
    const dim3 grid(ragged_grid(nf.longest, RW_THREADS, RW_MAX_GRID), (unsigned)nrec);
    hipLaunchKernelGGL(window_frames_stitch_kernel, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, rows, n_rows, stride, table,
                       frames, (int64_t)nwin, recs, ratios, core, context, nf.total, out);
    return sos_check_launch(who);
}

extern "C" int sos_window_frames_link_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table,
                                          const int64_t* table_host, const int64_t* frames, const int64_t* frames_host, int nwin,
                                          const int64_t* recs, const int64_t* recs_host, const double* ratios,
                                          const double* ratios_host, int nrec, int64_t core, int64_t context, const int64_t* links,
                                          const int64_t* links_host, const int64_t* members, const int64_t* members_host,
                                          int ngroups, int mode, float threshold, float* out_logits, uint8_t* out_bits,
                                          sos_stream_t stream) {
    const char* who = "sos_window_frames_link_f32";
    if (!frames_args_ok(who, rows, out_logits, table, table_host, frames, frames_host, nwin, recs, recs_host, ratios, ratios_host,
                        nrec, n_rows, stride, core, context))
        return SOS_EINVAL;
    if (!links || !links_host || !members || !members_host || !out_bits) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (ngroups < 1 || ngroups > RAGGED_MAX_CLIPS || (mode != 0 && mode != 1) || !std::isfinite(threshold)) {
        sos_set_error("%s: bad args (1 .. 65535 groups, got %d; mode %d, 0 = any or 1 = mean; threshold %g must be finite)", who,
                      ngroups, mode, (double)threshold);
        return SOS_EINVAL;
    }
    RaggedSum nf;
    int bad = ragged_sum_column(links_host, ngroups, RW_LINK_COLS, 1, 0, RW_MAX_FRAMES, &nf);
    if (bad < ngroups) {
        sos_set_error("%s: group %d has %lld frames (0 .. %lld)", who, bad, (long long)link_row(links_host, bad).F,
                      (long long)RW_MAX_FRAMES);
        return SOS_EINVAL;
    }
    // `members` holds what the groups count: every group's range must lie inside that
    int64_t nmem = 0;
    for (int g = 0; g < ngroups; ++g) {
        const LinkRow lk = link_row(links_host, g);
        if (lk.count < 1 || lk.count > nrec) {
            sos_set_error(lk.count == 0 ? "%s: group %d has no members (%lld; 1 .. %d, the recordings)"
                                        : "%s: group %d has a member count of %lld (1 .. %d, the recordings)", who, g,
                          (long long)lk.count, nrec);
            return SOS_EINVAL;
        }
        nmem += lk.count;
    }
    std::vector<std::pair<int64_t, int>> streams;              // {frame offset, group} of the groups that hold frames
    for (int g = 0; g < ngroups; ++g) {
        const LinkRow lk = link_row(links_host, g);
        if (!link_ok(lk, nmem, nf.total)) {
            sos_set_error("%s: group %d (frames %lld + %lld of %lld, members %lld + %lld of %lld) lies outside the summed output or "
                          "the members", who, g, (long long)lk.foff, (long long)lk.F, (long long)nf.total, (long long)lk.first,
                          (long long)lk.count, (long long)nmem);
            return SOS_EINVAL;
        }
        if (lk.F > 0) streams.push_back({lk.foff, g});
    }
    std::sort(streams.begin(), streams.end());
    for (size_t k = 1; k < streams.size(); ++k)
        if (streams[k].first < streams[k - 1].first + link_row(links_host, streams[k - 1].second).F) {
            sos_set_error("%s: group %d and group %d overlap in the output (frames from %lld and from %lld)", who,
                          streams[k - 1].second, streams[k].second, (long long)streams[k - 1].first, (long long)streams[k].first);
            return SOS_EINVAL;
        }
    std::vector<int> group_of(nrec, -1);
    for (int g = 0; g < ngroups; ++g) {
        const LinkRow lk = link_row(links_host, g);
        const double rho = ratios_host[std::min<int64_t>(std::max<int64_t>(members_host[lk.first], 0), nrec - 1)];
        for (int64_t m = 0; m < lk.count; ++m) {
            const int64_t r = members_host[lk.first + m];
            if (r < 0 || r >= nrec) {
                sos_set_error("%s: member %lld of group %d names recording %lld of %d", who, (long long)m, g, (long long)r, nrec);
                return SOS_EINVAL;
            }
            if (group_of[r] >= 0) {
                sos_set_error("%s: recording %lld appears twice, as member %lld of group %d and in group %d", who, (long long)r,
                              (long long)m, g, group_of[r]);
                return SOS_EINVAL;
            }
            group_of[r] = g;
            const FrameRec rec = frame_rec(recs_host, r);
            if (!frames_rec_windows_ok(rec, ratios_host[r], nwin)) {
                sos_set_error("%s: recording %lld, member %lld of group %d (frames %lld, windows %lld + %lld of %d, %g samples per "
                              "frame) lies outside the table, or has a ratio outside (0, 2^30]", who, (long long)r, (long long)m, g,
                              (long long)rec.F, (long long)rec.first, (long long)rec.K, nwin, ratios_host[r]);
                return SOS_EINVAL;
            }
            if (rec.F != lk.F || ratios_host[r] != rho) {
                sos_set_error("%s: recording %lld, member %lld of group %d, has %lld frames of %g samples; its group has %lld frames "
                              "and its first member %g samples per frame: the members of a group share one frame grid", who,
                              (long long)r, (long long)m, g, (long long)rec.F, ratios_host[r], (long long)lk.F, rho);
                return SOS_EINVAL;
            }
            if (!frames_windows_ok(who, (int)r, rec, table_host, frames_host, n_rows, stride)) return SOS_EINVAL;
        }
    }
    const dim3 grid(ragged_grid(nf.longest, RW_THREADS, RW_MAX_GRID), (unsigned)ngroups);
    hipLaunchKernelGGL(window_frames_link_kernel, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, rows, n_rows, stride, table,
                       frames, (int64_t)nwin, recs, ratios, (int64_t)nrec, links, members, nmem, core, context, mode, threshold,
                       nf.total, out_logits, out_bits);
    return sos_check_launch(who);
}

// ---- windows staged with the recording's mask

// window e of recording c (a row of the clip table): inside the stride, inside its recording, and its source offset is that
// recording's sample `start`
__host__ __device__ static inline bool window_masked_ok(const WindowRow& e, const RaggedClip& c, int64_t stride) {
    return e.n >= 0 && e.n <= stride && e.start >= 0 && e.n <= c.n && e.start <= c.n - e.n && e.off >= e.start && e.off - e.start == c.off;
}

__global__ __launch_bounds__(RW_THREADS) void window_stage_masked_kernel(
    const float* __restrict__ x, int64_t total, const uint8_t* __restrict__ bits, int64_t total_bits,
    const int64_t* __restrict__ clips, const double* __restrict__ ratios, int64_t nrec, const int64_t* __restrict__ table,
    int64_t stride, float* __restrict__ wave, float* __restrict__ masked) {
    const int64_t w = blockIdx.y;
    const WindowRow e = window_row(table, w);
    if (e.rec < 0 || e.rec >= nrec) return;
    const RaggedClip c = ragged_clip(clips, e.rec);
    const double ratio = ratios[e.rec];
    if (!ragged_row_inside(c, total, total_bits) || !(ratio > 1.0) || !window_masked_ok(e, c, stride)) return;
    const float* src = x + c.off + e.start;
    const uint8_t* bc = bits + c.foff;
    float* wrow = wave + w * stride;
    float* mrow = masked + w * stride;
    const int64_t n = e.n, g = e.start;                         // sample j of the window is sample g + j of the recording
    const bool row_vec = (stride & 3) == 0 && ragged_aligned16(wave) && ragged_aligned16(masked), src_vec = ragged_aligned16(src);
    for (int64_t j0 = ((int64_t)blockIdx.x * RW_THREADS + threadIdx.x) * 4; j0 < stride; j0 += (int64_t)gridDim.x * RW_THREADS * 4) {
        const bool full = j0 + 4 <= n;
        float v[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f};      // zero from the window's end to the stride
        ragged_load4(src, j0, n, full && src_vec, v);
        bool one = false;
        if (full) {
            // A quad whose samples all have their four left neighbours in the same frame interval [lo, hi) of mask_rule.h: each
            // lies in an original run of five or more equal values, which is never flipped, so all four take the frame's value --
            // what mask_sample returns for each of them, from one interval instead of four times three (5.5 % of the kernel's
            // time on 30 s windows at 30 fps, EXPERIMENTS.md 3.15).
            const int64_t i = (int64_t)((double)(g + j0) / ratio);
            if (i < c.frames) {
                const int64_t lo = frame_edge(i, ratio), hi = (int64_t)__dadd_rn(__dmul_rn((double)(i + 1), ratio), -1.0);
                if (g + j0 >= lo + 4 && g + j0 + 3 < hi) {
                    m[0] = m[1] = m[2] = m[3] = bc[i] == 0 ? 1.f : 0.f;
                    one = true;
                }
            }
        }
        if (!one) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < n) m[k] = mask_sample(bc, c.frames, ratio, c.n, g + j0 + k);
        }
        ragged_store4(wrow, j0, stride, row_vec, v);            // row_vec: the stride is a multiple of four, so j0 + 4 <= stride
        const float vm[4] = {v[0] * m[0], v[1] * m[1], v[2] * m[2], v[3] * m[3]};
        ragged_store4(mrow, j0, stride, row_vec, vm);
    }
}

extern "C" int sos_window_stage_masked_f32(const float* x, const uint8_t* bits, const int64_t* clips, const int64_t* clips_host,
                                           const double* ratios, const double* ratios_host, int nrec, const int64_t* table,
                                           const int64_t* table_host, int nwin, int64_t stride, float* wave, float* masked,
                                           sos_stream_t stream) {
    const char* who = "sos_window_stage_masked_f32";
    if (!window_args_ok(who, x, wave, table, table_host, nwin, stride)) return SOS_EINVAL;
    if (!bits || !clips || !clips_host || !ratios || !ratios_host || !masked) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (nrec < 1 || nrec > RAGGED_MAX_CLIPS) {
        sos_set_error("%s: bad args (1 .. 65535 recordings, got %d)", who, nrec);
        return SOS_EINVAL;
    }
    RaggedSum ns, nf;
    int bad = std::min(ragged_sum_column(clips_host, nrec, RAGGED_CLIP_COLS, 1, 0, INT64_MAX / 8, &ns),
                       ragged_sum_column(clips_host, nrec, RAGGED_CLIP_COLS, 3, 0, INT64_MAX / 8, &nf));
    if (bad < nrec) {
        const RaggedClip c = ragged_clip(clips_host, bad);
        sos_set_error("%s: recording %d has %lld samples and %lld frames", who, bad, (long long)c.n, (long long)c.frames);
        return SOS_EINVAL;
    }
    for (int r = 0; r < nrec; ++r) {
        const RaggedClip c = ragged_clip(clips_host, r);
        if (!ragged_row_inside(c, ns.total, nf.total)) {
            sos_set_error("%s: recording %d (samples %lld + %lld, frames %lld + %lld) lies outside the %lld samples / %lld frames "
                          "of the table", who, r, (long long)c.off, (long long)c.n, (long long)c.foff, (long long)c.frames,
                          (long long)ns.total, (long long)nf.total);
            return SOS_EINVAL;
        }
        if (!(ratios_host[r] > 1.0)) {
            sos_set_error("%s: recording %d has ratio %g (samples per frame must exceed 1)", who, r, ratios_host[r]);
            return SOS_EINVAL;
        }
    }
    for (int w = 0; w < nwin; ++w) {
        const WindowRow e = window_row(table_host, w);
        if (e.n > stride) {
            sos_set_error("%s: window %d has %lld samples (stride %lld)", who, w, (long long)e.n, (long long)stride);
            return SOS_EINVAL;
        }
        if (e.rec < 0 || e.rec >= nrec || !window_masked_ok(e, ragged_clip(clips_host, e.rec), stride)) {
            sos_set_error("%s: window %d (recording %lld of %d, source offset %lld, start %lld, samples %lld) lies outside its "
                          "recording, or its source offset is not its start in that recording", who, w, (long long)e.rec, nrec,
                          (long long)e.off, (long long)e.start, (long long)e.n);
            return SOS_EINVAL;
        }
    }
    const dim3 grid(ragged_grid((stride + 3) / 4, RW_THREADS, RW_MAX_GRID), (unsigned)nwin);
    hipLaunchKernelGGL(window_stage_masked_kernel, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, x, ns.total, bits, nf.total,
                       clips, ratios, (int64_t)nrec, table, stride, wave, masked);
    return sos_check_launch(who);
}
