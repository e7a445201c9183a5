// stream_window.hip -- the three copies around "live audio denoised in windows" (pipeline.StreamDenoiser; the rule is
// pipeline.StreamPlan, its float64 restatement tests/stream_reference.py).  What ragged_window.hip does for recordings that are
// complete, these do for streams that arrive in chunks; the state between two calls stays on the device:
//   ring [slots][cap]           the samples of a stream that have arrived and belong to no finished window yet: sample p of the
//                               stream lies at ring[slot][p % cap]
//   tail [slots][2][2 context]  the overlap [b - context, b + context) of the last window's row around its core end b, which the
//                               next window is blended with.  Two halves: a stitch reads half `parity` and writes half
//                               `parity ^ 1`, so no thread of a launch reads what another one of it writes.
//   stream_push_kernel     chunks lying back to back in one buffer -> each into its slot's ring at its stream position.
//   stream_stage_kernel    window_stage_kernel with a modular source index: one zero-filled row per window out of the rings.
//   stream_stitch_kernel   one row per window -> the samples that are final after it, [core start - context, core end - context)
//                          (from the core start without a previous window, to the core end without a next one), the first
//                          2 context of them blended with the saved overlap by window_quad's f32 statement
//                              w = (i + 0.5) / (2 context),  out = (1 - w) earlier + w later,
//                          and the window's own overlap saved for the next call.  What it emits for a stream, call after call,
//                          is bit for bit what window_stitch_kernel writes for the whole recording.
// One launch each whatever the number of slots; a thread handles four consecutive samples, one 16-byte access where the address
// allows it and scalar accesses otherwise (which of the two is taken changes no value); no atomics.
// Bounds: the rule of ragged.h -- the host refuses a row that leaves what the buffers hold (SOS_EINVAL, the row is named), the
// kernels skip a row of the DEVICE table that fails the same test (stream_push_ok / stream_stage_ok / stream_stitch_why).  A
// slot named twice in one table is a race, not an access out of bounds: the host refuses it, the kernels cannot see it.
#include "ragged.h"
#include <vector>

#define SW_THREADS 256
#define SW_MAX_GRID 1024                // workgroups along a row (they stride over what the grid does not cover)
#define SW_STITCH_QUADS 4               // quads per thread the stitch grid is sized for
#define SW_PUSH_COLS 4                  // int64 per chunk
#define SW_STAGE_COLS 3                 // int64 per staged window
#define SW_STITCH_COLS 8                // int64 per stitched window
#define SW_MAX_CONTEXT ((int64_t)1 << 22)   // 2 context + 0.5 is exact in f32 (RW_MAX_CONTEXT of ragged_window.hip)
#define SW_HAS_PREV 1                   // flags: a window ran before this one (blend with the saved overlap)
#define SW_HAS_NEXT 2                   // ... one will run after it (hold the last `context` back, save the overlap)

__host__ __device__ static inline bool stream_small(int64_t v) { return v >= 0 && v <= INT64_MAX / 8; }

// A chunk: `n` samples from flat[off] on are the samples pos .. pos + n of stream `slot`.
struct StreamPush { int64_t slot, off, n, pos; };
__host__ __device__ static inline StreamPush stream_push_row(const int64_t* table, int64_t r) {
    const int64_t* te = table + r * SW_PUSH_COLS;
    return {te[0], te[1], te[2], te[3]};
}
__host__ __device__ static inline bool stream_push_ok(const StreamPush& e, int64_t slots, int64_t cap, int64_t total) {
    return e.slot >= 0 && e.slot < slots && e.n <= cap && stream_small(e.pos) && ragged_clip_inside(e.off, e.n, total);
}

// A window to stage: the samples start .. start + n of stream `slot`.
struct StreamStage { int64_t slot, start, n; };
__host__ __device__ static inline StreamStage stream_stage_row(const int64_t* table, int64_t w) {
    const int64_t* te = table + w * SW_STAGE_COLS;
    return {te[0], te[1], te[2]};
}
__host__ __device__ static inline bool stream_stage_ok(const StreamStage& e, int64_t slots, int64_t cap, int64_t stride) {
    return e.slot >= 0 && e.slot < slots && e.n >= 0 && e.n <= cap && e.n <= stride && stream_small(e.start);
}

// A window to stitch.  row: its row in `rows`, holding n samples from sample `start` of the stream on; cs, ce: its core.
struct StreamStitch { int64_t slot, row, start, n, cs, ce, flags, parity; };
__host__ __device__ static inline StreamStitch stream_stitch_row(const int64_t* table, int64_t w) {
    const int64_t* te = table + w * SW_STITCH_COLS;
    return {te[0], te[1], te[2], te[3], te[4], te[5], te[6], te[7]};
}
// the samples the window makes final: [lo, hi) of the stream
__host__ __device__ static inline int64_t stream_emit_lo(const StreamStitch& e, int64_t context) {
    return (e.flags & SW_HAS_PREV) ? e.cs - context : e.cs;
}
__host__ __device__ static inline int64_t stream_emit_hi(const StreamStitch& e, int64_t context) {
    return (e.flags & SW_HAS_NEXT) ? e.ce - context : e.ce;
}
// Why a row of a stitch table cannot be followed (0: it can).  Every comparison is between values already known to lie in
// [0, INT64_MAX / 8], so no sum overflows.
enum { SW_OK = 0, SW_SLOT, SW_ROW, SW_SAMPLES, SW_CORE, SW_FLAGS, SW_CONTEXT, SW_OVERLAP, SW_OUTPUT };
__host__ __device__ static inline int stream_stitch_why(const StreamStitch& e, int64_t slots, int64_t n_rows, int64_t stride,
                                                        int64_t out_stride, int64_t context) {
    if (e.slot < 0 || e.slot >= slots) return SW_SLOT;
    if (e.row < 0 || e.row >= n_rows) return SW_ROW;
    if (e.n < 0 || e.n > stride) return SW_SAMPLES;
    // the core lies inside the row's own samples
    if (!stream_small(e.start) || !stream_small(e.cs) || !stream_small(e.ce) || e.start > e.cs || e.cs > e.ce || e.ce - e.start > e.n)
        return SW_CORE;
    if (e.flags < 0 || e.flags > (SW_HAS_PREV | SW_HAS_NEXT) || e.parity < 0 || e.parity > 1) return SW_FLAGS;
    const bool prev = (e.flags & SW_HAS_PREV) != 0, next = (e.flags & SW_HAS_NEXT) != 0;
    if (((int)prev + (int)next) * context > e.ce - e.cs) return SW_CONTEXT;
    // the overlaps [cs - context, cs + context) and [ce - context, ce + context) lie inside the row
    if ((prev && e.cs - e.start < context) || (next && e.n - (e.ce - e.start) < context)) return SW_OVERLAP;
    if (stream_emit_hi(e, context) - stream_emit_lo(e, context) > out_stride) return SW_OUTPUT;
    return SW_OK;
}

// v[k] = p[j0 + k] for j0 + k < end: one 16-byte load where all four are wanted and the address allows it
__device__ __forceinline__ void stream_load4(const float* p, int64_t j0, int64_t end, float (&v)[4]) {
    ragged_load4(p, j0, end, j0 + 4 <= end && ragged_aligned16(p + j0), v);
}
__device__ __forceinline__ void stream_store4(float* p, int64_t j0, int64_t end, const float (&v)[4]) {
    ragged_store4(p, j0, end, j0 + 4 <= end && ragged_aligned16(p + j0), v);
}
// The same for `left` samples of a ring of `cap` floats from element p0 < cap on, wrapping round its end.
__device__ __forceinline__ void stream_ring_load4(const float* ring, int64_t cap, int64_t p0, int64_t left, float (&v)[4]) {
    if (left >= 4 && p0 + 4 <= cap && ragged_aligned16(ring + p0)) {
        const ragged_f32x4 q = *(const ragged_f32x4*)(ring + p0);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < left) v[k] = ring[p0 + k < cap ? p0 + k : p0 + k - cap];
    }
}
__device__ __forceinline__ void stream_ring_store4(float* ring, int64_t cap, int64_t p0, int64_t left, const float (&v)[4]) {
    if (left >= 4 && p0 + 4 <= cap && ragged_aligned16(ring + p0)) {
        *(ragged_f32x4*)(ring + p0) = ragged_f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < left) ring[p0 + k < cap ? p0 + k : p0 + k - cap] = v[k];
    }
}

__global__ __launch_bounds__(SW_THREADS) void stream_push_kernel(const float* __restrict__ flat, int64_t total,
                                                                const int64_t* __restrict__ table, float* __restrict__ ring,
                                                                int64_t slots, int64_t cap) {
    const StreamPush e = stream_push_row(table, blockIdx.y);
    if (!stream_push_ok(e, slots, cap, total)) return;
    const float* src = flat + e.off;
    float* dst = ring + e.slot * cap;
    const int64_t n = e.n, base = e.pos % cap;
    const bool src_vec = ragged_aligned16(src);
    for (int64_t j0 = ((int64_t)blockIdx.x * SW_THREADS + threadIdx.x) * 4; j0 < n; j0 += (int64_t)gridDim.x * SW_THREADS * 4) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        ragged_load4(src, j0, n, j0 + 4 <= n && src_vec, v);
        const int64_t p0 = base + j0 < cap ? base + j0 : base + j0 - cap;       // j0 < n <= cap
        stream_ring_store4(dst, cap, p0, n - j0, v);
    }
}

__global__ __launch_bounds__(SW_THREADS) void stream_stage_kernel(const float* __restrict__ ring, int64_t slots, int64_t cap,
                                                                 const int64_t* __restrict__ table, int64_t stride,
                                                                 float* __restrict__ rows) {
    const int64_t w = blockIdx.y;
    const StreamStage e = stream_stage_row(table, w);
    if (!stream_stage_ok(e, slots, cap, stride)) return;
    const float* src = ring + e.slot * cap;
    float* dst = rows + w * stride;
    const int64_t n = e.n, base = e.start % cap;
    const bool row_vec = (stride & 3) == 0 && ragged_aligned16(rows);
    for (int64_t j0 = ((int64_t)blockIdx.x * SW_THREADS + threadIdx.x) * 4; j0 < stride; j0 += (int64_t)gridDim.x * SW_THREADS * 4) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};                      // zero from the window's end to the stride
        if (j0 < n) stream_ring_load4(src, cap, base + j0 < cap ? base + j0 : base + j0 - cap, n - j0, v);
        ragged_store4(dst, j0, stride, row_vec, v);             // row_vec: the stride is a multiple of four, so j0 + 4 <= stride
    }
}

__global__ __launch_bounds__(SW_THREADS) void stream_stitch_kernel(const float* __restrict__ rows, int64_t n_rows, int64_t stride,
                                                                  const int64_t* __restrict__ table, int64_t slots,
                                                                  int64_t context, float* __restrict__ tail,
                                                                  float* __restrict__ out, int64_t out_stride) {
    const int64_t w = blockIdx.y;
    const StreamStitch e = stream_stitch_row(table, w);
    if (stream_stitch_why(e, slots, n_rows, stride, out_stride, context) != SW_OK) return;
    const int64_t lo = stream_emit_lo(e, context), len = stream_emit_hi(e, context) - lo, zone = 2 * context;
    const float* row = rows + e.row * stride;
    const float* own = row + (lo - e.start);                    // sample j of what is emitted
    const float* earlier = tail + (e.slot * 2 + e.parity) * zone;
    const int64_t head = (e.flags & SW_HAS_PREV) ? zone : 0;    // sample j < head blends with the saved overlap
    float* dst = out + w * out_stride;
    const float span = (float)zone;
    const int64_t j_first = ((int64_t)blockIdx.x * SW_THREADS + threadIdx.x) * 4, j_step = (int64_t)gridDim.x * SW_THREADS * 4;
    for (int64_t j0 = j_first; j0 < len; j0 += j_step) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        stream_load4(own, j0, len, v);
        if (j0 < head) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            stream_load4(earlier, j0, head, a);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < head) {
                    const float wt = ((float)(j0 + k) + 0.5f) / span;
                    v[k] = (1.f - wt) * a[k] + wt * v[k];
                }
        }
        stream_store4(dst, j0, len, v);
    }
    if (!(e.flags & SW_HAS_NEXT)) return;
    const float* keep = row + (e.ce - context - e.start);       // the overlap around this window's core end, for the next call
    float* later = tail + (e.slot * 2 + (e.parity ^ 1)) * zone;
    for (int64_t j0 = j_first; j0 < zone; j0 += j_step) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        stream_load4(keep, j0, zone, v);
        stream_store4(later, j0, zone, v);
    }
}

static bool stream_args_ok(const char* who, const void* a, const void* b, const int64_t* table, const int64_t* table_host, int nrows,
                           int64_t slots, int64_t cap) {
    if (!a || !b || !table || !table_host) { sos_set_error("%s: null pointer", who); return false; }
    if (nrows < 1 || nrows > RAGGED_MAX_CLIPS || slots < 1 || slots > RAGGED_MAX_CLIPS || cap < 1 ||
        cap > INT64_MAX / 8 / RAGGED_MAX_CLIPS) {
        sos_set_error("%s: bad args (1 .. 65535 rows, got %d; 1 .. 65535 slots, got %lld; a ring of %lld samples)", who, nrows,
                      (long long)slots, (long long)cap);
        return false;
    }
    return true;
}

// false with the error set if row r names a slot outside the slots or one that an earlier row named
static bool stream_slot_once(const char* who, std::vector<uint8_t>& seen, int r, int64_t slot) {
    if (slot < 0 || slot >= (int64_t)seen.size()) {
        sos_set_error("%s: row %d names slot %lld of %lld", who, r, (long long)slot, (long long)seen.size());
        return false;
    }
    if (seen[slot]) {
        sos_set_error("%s: row %d names slot %lld, which an earlier row of the table names", who, r, (long long)slot);
        return false;
    }
    seen[slot] = 1;
    return true;
}

extern "C" int sos_stream_push_f32(const float* flat, int64_t total, const int64_t* table, const int64_t* table_host, int nrows,
                                   float* ring, int64_t slots, int64_t cap, sos_stream_t stream) {
    const char* who = "sos_stream_push_f32";
    if (!stream_args_ok(who, flat, ring, table, table_host, nrows, slots, cap)) return SOS_EINVAL;
    if (total < 0 || total > INT64_MAX / 8) {
        sos_set_error("%s: a buffer of %lld samples", who, (long long)total);
        return SOS_EINVAL;
    }
    std::vector<uint8_t> seen(slots, 0);
    int64_t longest = 0;
    for (int r = 0; r < nrows; ++r) {
        const StreamPush e = stream_push_row(table_host, r);
        if (!stream_slot_once(who, seen, r, e.slot)) return SOS_EINVAL;
        if (e.n > cap) {
            sos_set_error("%s: row %d has %lld samples (a ring holds %lld)", who, r, (long long)e.n, (long long)cap);
            return SOS_EINVAL;
        }
        if (!stream_small(e.pos)) {
            sos_set_error("%s: row %d writes at the stream position %lld", who, r, (long long)e.pos);
            return SOS_EINVAL;
        }
        if (!stream_push_ok(e, slots, cap, total)) {
            sos_set_error("%s: row %d (samples %lld + %lld) lies outside the %lld samples of the buffer", who, r, (long long)e.off,
                          (long long)e.n, (long long)total);
            return SOS_EINVAL;
        }
        longest = std::max(longest, e.n);
    }
    const dim3 grid(ragged_grid((longest + 3) / 4, SW_THREADS, SW_MAX_GRID), (unsigned)nrows);
    hipLaunchKernelGGL(stream_push_kernel, grid, dim3(SW_THREADS), 0, (hipStream_t)stream, flat, total, table, ring, slots, cap);
    return sos_check_launch(who);
}

extern "C" int sos_stream_stage_f32(const float* ring, int64_t slots, int64_t cap, const int64_t* table, const int64_t* table_host,
                                    int nwin, int64_t stride, float* rows, sos_stream_t stream) {
    const char* who = "sos_stream_stage_f32";
    if (!stream_args_ok(who, ring, rows, table, table_host, nwin, slots, cap)) return SOS_EINVAL;
    if (stride < 1 || stride > INT64_MAX / 8 / RAGGED_MAX_CLIPS) {
        sos_set_error("%s: bad args (stride %lld)", who, (long long)stride);
        return SOS_EINVAL;
    }
    for (int w = 0; w < nwin; ++w) {
        const StreamStage e = stream_stage_row(table_host, w);
        if (e.slot < 0 || e.slot >= slots) {
            sos_set_error("%s: row %d names slot %lld of %lld", who, w, (long long)e.slot, (long long)slots);
            return SOS_EINVAL;
        }
        if (e.n < 0 || e.n > stride || e.n > cap) {
            sos_set_error("%s: row %d has %lld samples (stride %lld, a ring holds %lld)", who, w, (long long)e.n, (long long)stride,
                          (long long)cap);
            return SOS_EINVAL;
        }
        if (!stream_stage_ok(e, slots, cap, stride)) {
            sos_set_error("%s: row %d starts at the stream position %lld", who, w, (long long)e.start);
            return SOS_EINVAL;
        }
    }
    const dim3 grid(ragged_grid((stride + 3) / 4, SW_THREADS, SW_MAX_GRID), (unsigned)nwin);
    hipLaunchKernelGGL(stream_stage_kernel, grid, dim3(SW_THREADS), 0, (hipStream_t)stream, ring, slots, cap, table, stride, rows);
    return sos_check_launch(who);
}

extern "C" int sos_stream_stitch_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table,
                                     const int64_t* table_host, int nwin, int64_t slots, int64_t context, float* tail, float* out,
                                     int64_t out_stride, sos_stream_t stream) {
    const char* who = "sos_stream_stitch_f32";
    if (!stream_args_ok(who, rows, out, table, table_host, nwin, slots, 1)) return SOS_EINVAL;
    if (!tail) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (stride < 1 || stride > INT64_MAX / 8 / RAGGED_MAX_CLIPS || n_rows < 1 || n_rows > INT64_MAX / 8 / stride || out_stride < 1 ||
        out_stride > INT64_MAX / 8 / RAGGED_MAX_CLIPS || context < 0 || context > SW_MAX_CONTEXT) {
        sos_set_error("%s: bad args (%lld rows of %lld; an output stride of %lld; context %lld, 0 .. %lld)", who, (long long)n_rows,
                      (long long)stride, (long long)out_stride, (long long)context, (long long)SW_MAX_CONTEXT);
        return SOS_EINVAL;
    }
    std::vector<uint8_t> seen(slots, 0);
    for (int w = 0; w < nwin; ++w) {
        const StreamStitch e = stream_stitch_row(table_host, w);
        const int why = stream_stitch_why(e, slots, n_rows, stride, out_stride, context);
        if (why == SW_OK || why == SW_SLOT) {
            if (!stream_slot_once(who, seen, w, e.slot)) return SOS_EINVAL;
            continue;
        }
        static const char* const reason[] = {"", "", "names a row outside the rows", "has more samples than the stride",
                                             "has a core outside its own samples", "has flags outside 0 .. 3 or a parity outside 0 .. 1",
                                             "blends over more context than its core holds", "has an overlap outside its own samples",
                                             "emits more samples than the output stride"};
        sos_set_error("%s: row %d %s (slot %lld, row %lld of %lld, samples %lld, stride %lld, start %lld, core %lld .. %lld, flags "
                      "%lld, parity %lld, context %lld, output stride %lld)", who, w, reason[why], (long long)e.slot, (long long)e.row,
                      (long long)n_rows, (long long)e.n, (long long)stride, (long long)e.start, (long long)e.cs, (long long)e.ce,
                      (long long)e.flags, (long long)e.parity, (long long)context, (long long)out_stride);
        return SOS_EINVAL;
    }
    // the grid follows nwin, the strides and the context alone: four quads per thread as in sos_window_stitch_f32
    const dim3 grid(ragged_grid((std::max(out_stride, 2 * context) + 3) / 4, SW_THREADS * SW_STITCH_QUADS, SW_MAX_GRID), (unsigned)nwin);
    hipLaunchKernelGGL(stream_stitch_kernel, grid, dim3(SW_THREADS), 0, (hipStream_t)stream, rows, n_rows, stride, table, slots,
                       context, tail, out, out_stride);
    return sos_check_launch(who);
}
