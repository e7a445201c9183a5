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
// Bounds: the rule of ragged.h -- the host refuses a table entry that leaves what it sized from table_host (SOS_EINVAL), the
// kernels skip an entry of the DEVICE table that fails the same test (window_stage_ok / window_stitch_why below).
#include "ragged.h"

#define RW_THREADS 256
#define RW_MAX_GRID 1024                // workgroups along a row (they stride over what the grid does not cover)
#define RW_STITCH_QUADS 4               // quads per thread the stitch grid is sized for
#define RW_COLS 10                      // int64 per window, the row of pipeline.window_plan
#define RW_MAX_CONTEXT ((int64_t)1 << 22)   // 2 context + 0.5 is exact in f32

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
    // the zones: j < head blends with the window before, j >= tail with the window after
    const int64_t head = context > 0 && e.prev >= 0 ? context : 0, tail = context > 0 && e.next >= 0 ? len - context : len;
    int64_t before = 0, after = 0;                              // element of `rows` that holds sample cs of the neighbour's row
    if (head) {
        const WindowRow q = window_row(table, e.prev);
        before = q.row * stride + (e.cs - q.start);
    }
    if (tail < len) {
        const WindowRow q = window_row(table, e.next);
        after = q.row * stride + (e.cs - q.start);              // negative for a while: only j >= tail is read
    }
    const float span = (float)(2 * context);
    for (int64_t j0 = ((int64_t)blockIdx.x * RW_THREADS + threadIdx.x) * 4; j0 < len; j0 += (int64_t)gridDim.x * RW_THREADS * 4) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        window_load4(rows, own + j0, j0, 0, len, v);
        if (j0 < head) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            window_load4(rows, before + j0, j0, 0, head, a);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < head) {
                    const float wt = ((float)(j0 + k + context) + 0.5f) / span;
                    v[k] = (1.f - wt) * a[k] + wt * v[k];
                }
        }
        if (j0 + 4 > tail) {
            float b[4] = {0.f, 0.f, 0.f, 0.f};
            window_load4(rows, after + j0, j0, tail, len, b);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k >= tail && j0 + k < len) {
                    const float wt = ((float)(j0 + k - tail) + 0.5f) / span;
                    v[k] = (1.f - wt) * v[k] + wt * b[k];
                }
        }
        ragged_store4(dst, j0, len, j0 + 4 <= len && dst_vec, v);
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

extern "C" int sos_window_stitch_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table,
                                     const int64_t* table_host, int nwin, int64_t context, float* out, sos_stream_t stream) {
    if (!window_args_ok("sos_window_stitch_f32", rows, out, table, table_host, nwin, stride)) return SOS_EINVAL;
    if (n_rows < 1 || n_rows > INT64_MAX / 8 / stride || context < 0 || context > RW_MAX_CONTEXT) {
        sos_set_error("sos_window_stitch_f32: bad args (%lld rows of %lld; context %lld, 0 .. %lld)", (long long)n_rows,
                      (long long)stride, (long long)context, (long long)RW_MAX_CONTEXT);
        return SOS_EINVAL;
    }
    // the summed output length: the cores tile the recordings' outputs
    int64_t total_out = 0, longest = 0;
    for (int w = 0; w < nwin; ++w) {
        const WindowRow e = window_row(table_host, w);
        if (!window_small(e.cs) || !window_small(e.ce) || e.cs > e.ce || e.ce - e.cs > INT64_MAX / 8 - total_out) {
            sos_set_error("sos_window_stitch_f32: window %d has the core %lld .. %lld", w, (long long)e.cs, (long long)e.ce);
            return SOS_EINVAL;
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
        sos_set_error("sos_window_stitch_f32: window %d %s (row %lld of %lld, samples %lld, stride %lld, start %lld, core %lld .. "
                      "%lld, output %lld of %lld, neighbours %lld and %lld, context %lld)", w, reason[why], (long long)e.row,
                      (long long)n_rows, (long long)e.n, (long long)stride, (long long)e.start, (long long)e.cs, (long long)e.ce,
                      (long long)e.out, (long long)total_out, (long long)e.prev, (long long)e.next, (long long)context);
        return SOS_EINVAL;
    }
    // four quads per thread: a workgroup reads its row and both neighbours' before its first sample, which few samples do not repay
    const dim3 grid(ragged_grid((longest + 3) / 4, RW_THREADS * RW_STITCH_QUADS, RW_MAX_GRID), (unsigned)nwin);
    hipLaunchKernelGGL(window_stitch_kernel, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, rows, n_rows, stride, table,
                       (int64_t)nwin, context, total_out, out);
    return sos_check_launch("sos_window_stitch_f32");
}
