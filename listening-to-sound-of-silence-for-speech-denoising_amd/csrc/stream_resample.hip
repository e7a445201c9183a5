// stream_resample.hip -- the band-limited resampler of wave_io.hip for audio that arrives in chunks
// (audio_io.StreamResampler; the rule and its float64 restatement: tests/stream_resample_reference.py).
//
// Output t of a signal depends on the signal's length only through the right wing's bound n_in - n(t) - 1, and neither wing
// reads more than R = nwin / index_step samples.  So once a stream has received n_recv samples, every t with
// n(t) + 1 + R <= n_recv is final: computed with n_in = n_recv it has the bits it has for any longer length.  After the outputs
// [0, T) only the samples from max(n(T) - (R - 1), 0) on are still needed; they stay in the stream's ring on the device
// (ring[slot][p % cap] holds sample p: what sos_stream_push_f32 of stream_window.hip writes).
//   sos_stream_resample_ready   host only: T and the first retained sample after n_recv samples, from the same running sum
//                               the kernel evaluates (a count that disagreed with the device by one where time(t) crosses an
//                               integer would emit a sample that is not final)
//   stream_resample_kernel      one launch whatever the number of slots: row r of a table = the outputs [t_lo, t_hi) of one
//                               slot's stream -> out[out_off ..], each by rs_output (resample_core.h) with a modular index, so
//                               bit for bit what resample_kernel writes for the whole signal
// Tile shape: the window in LDS (128 KB) leaves room for one workgroup per CU, as in resample_batch_kernel: the grid is at
// most one workgroup per CU, each loads the window once and walks the (row, SRS_TILE outputs) tiles gridDim.x apart.  A live
// push is small (100 ms at 48 kHz are 1 400 outputs per slot), so a tile is 256 outputs, one per thread, not the 4 096 of the
// file path: a single slot still spreads over six CUs.  The bits do not depend on it.
// Bounds: the rule of ragged.h -- the host refuses a row that leaves what the buffers hold (SOS_EINVAL, the row is named), the
// kernel skips a row of the DEVICE table that fails the same test (stream_rs_why).  The ring index is modular and so never
// leaves the slot's ring; the test of the span keeps a row from reading samples the ring no longer holds.  No atomics.
#include "resample_launch.h"
#include <stdlib.h>

#define SRS_THREADS 256
#define SRS_TILE 256                    // outputs per workgroup step (<= SRS_THREADS)
#define SRS_COLS 6                      // int64 per row
#define SRS_MAX_POS ((int64_t)1 << 52)  // stream positions and output counts: exact in f64

// A row: the outputs [t_lo, t_hi) of stream `slot`, computed as of a signal of n_in samples (t >= n_valid: zero).
struct StreamRs { int64_t slot, t_lo, t_hi, n_in, n_valid, out_off; };
__host__ __device__ static inline StreamRs stream_rs_row(const int64_t* table, int64_t r) {
    const int64_t* te = table + r * SRS_COLS;
    return {te[0], te[1], te[2], te[3], te[4], te[5]};
}

// Why a row cannot be followed (0: it can).  max_t: the outputs the time register `seg` describes; reach = R.
enum { SRS_OK = 0, SRS_SLOT, SRS_RANGE, SRS_VALID, SRS_OUTPUT, SRS_SPAN };
__host__ __device__ static inline int stream_rs_why(const StreamRs& e, int64_t slots, int64_t cap, int64_t total, int64_t max_t,
                                                    double ratio, int64_t reach, const RsSegs& seg) {
    if (e.slot < 0 || e.slot >= slots) return SRS_SLOT;
    if (e.t_lo < 0 || e.t_lo > e.t_hi || e.t_hi > max_t) return SRS_RANGE;
    if (e.n_in < 0 || e.n_in > SRS_MAX_POS || e.n_valid < 0 || e.n_valid > (int64_t)((double)e.n_in * ratio)) return SRS_VALID;
    if (!ragged_clip_inside(e.out_off, e.t_hi - e.t_lo, total)) return SRS_OUTPUT;
    const int64_t t_end = e.t_hi < e.n_valid ? e.t_hi : e.n_valid;
    if (e.t_lo < t_end) {
        // the samples read: from n(t_lo) - (R - 1) on, none at or past n_in; the ring holds the last `cap` before n_in
        const int64_t first = (int64_t)rs_time(seg, e.t_lo) - (reach - 1), last = (int64_t)rs_time(seg, t_end - 1);
        if (last >= e.n_in || e.n_in - (first > 0 ? first : 0) > cap) return SRS_SPAN;
    }
    return SRS_OK;
}
__host__ __device__ static inline int64_t stream_rs_tiles(const StreamRs& e, int tile) { return (e.t_hi - e.t_lo + tile - 1) / tile; }

__global__ __launch_bounds__(SRS_THREADS) void stream_resample_kernel(const float* __restrict__ ring, int64_t slots, int64_t cap,
                                                                     const int64_t* __restrict__ table, int nrows, int64_t total,
                                                                     int64_t max_t, double ratio, RsSegs seg, double scale,
                                                                     const float* __restrict__ win, int nwin, int num_table,
                                                                     int index_step, int tile_outputs, float* __restrict__ out) {
    extern __shared__ float w[];
    rs_load_window<SRS_THREADS>(w, win, nwin);
    const int64_t reach = nwin / index_step;
    // the tiles of the rows lie back to back in table order; this workgroup's tiles ascend, so one pass over the rows serves all
    int r = 0;
    bool read = false;
    int64_t tile0 = 0, tiles = 0;
    StreamRs e = {};
    for (int64_t tile = blockIdx.x;; tile += gridDim.x) {
        for (; r < nrows; tile0 += tiles, ++r, read = false) {
            if (!read) {
                e = stream_rs_row(table, r);
                tiles = stream_rs_why(e, slots, cap, total, max_t, ratio, reach, seg) == SRS_OK ? stream_rs_tiles(e, tile_outputs) : 0;
                read = true;
            }
            if (tile < tile0 + tiles) break;
        }
        if (r == nrows) return;
        const int64_t t = e.t_lo + (tile - tile0) * tile_outputs + threadIdx.x;
        if ((int)threadIdx.x < tile_outputs && t < e.t_hi)
            out[e.out_off + (t - e.t_lo)] =
                t < e.n_valid ? rs_output(RsRing{ring + e.slot * cap, cap}, e.n_in, seg, scale, w, nwin, num_table, index_step, t) : 0.f;
    }
}

extern "C" int sos_stream_resample_ready(double ratio, int nwin, int num_table, int64_t n_recv, int64_t* t_ready, int64_t* base) {
    const char* who = "sos_stream_resample_ready";
    RsFilter f;
    if (!t_ready || !base) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (!rs_filter(who, ratio, nwin, num_table, false, &f)) return SOS_EINVAL;
    if (n_recv < 0 || n_recv > SRS_MAX_POS) {
        sos_set_error("%s: a stream of %lld samples", who, (long long)n_recv);
        return SOS_EINVAL;
    }
    const int64_t reach = f.reach;                   // R
    *t_ready = *base = 0;
    if (n_recv <= reach) return SOS_OK;              // output 0 reads up to sample R
    // t is final iff n(t) + 1 + R <= n_recv, i.e. time(t) < n_recv - R: T = the first t whose time is not below that
    const double bound = (double)(n_recv - reach);
    RsSegs g;
    long long k_end = 0;
    if (const int rc = rs_segments(who, ratio, (int64_t)SRS_MAX_POS * 4, &g, bound, &k_end)) return rc;
    int64_t lo = 0, hi = k_end;                       // time is increasing, time(0) = 0 < bound <= time(k_end)
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (rs_time(g, mid) < bound) lo = mid; else hi = mid;
    }
    *t_ready = hi;
    const int64_t first = (int64_t)rs_time(g, hi) - (reach - 1);
    *base = first > 0 ? first : 0;
    return SOS_OK;
}

extern "C" int sos_stream_resample_f32(const float* ring, int64_t slots, int64_t cap, const int64_t* table, const int64_t* table_host,
                                       int nrows, double ratio, const float* win, int nwin, int num_table, float* out, int64_t total,
                                       sos_stream_t stream) {
    const char* who = "sos_stream_resample_f32";
    if (!ring || !table || !table_host || !win || !out) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (!rs_rings(who, nrows, slots, 1, cap)) return SOS_EINVAL;
    if (total < 0 || total > INT64_MAX / 8) { sos_set_error("%s: an output of %lld", who, (long long)total); return SOS_EINVAL; }
    RsFilter f;
    if (!rs_filter(who, ratio, nwin, num_table, true, &f)) return SOS_EINVAL;
    RsSegs seg;
    int64_t max_t;
    const auto t_hi = [table_host](int r) { return stream_rs_row(table_host, r).t_hi; };
    if (const int rc = rs_row_segments(who, nrows, t_hi, ratio, &seg, &max_t)) return rc;
    // tile shape: A/B switch, read per call (tools/stream_resample_bench.py flips it).  The results do not depend on it.
    const char* env_tile = getenv("SOS_STREAM_RESAMPLE_TILE");
    int tile = env_tile ? atoi(env_tile) : SRS_TILE;
    if (tile < 1 || tile > SRS_THREADS) tile = SRS_TILE;
    RsSlotsOnce once(slots);
    int64_t total_tiles = 0;
    for (int r = 0; r < nrows; ++r) {
        const StreamRs e = stream_rs_row(table_host, r);
        const int why = stream_rs_why(e, slots, cap, total, max_t, ratio, f.reach, seg);
        if (why == SRS_OK) {
            if (!once.take(who, r, e.slot)) return SOS_EINVAL;
            total_tiles += stream_rs_tiles(e, tile);
            continue;
        }
        static const char* const reason[] = {"", "names a slot outside the slots", "has outputs that are no range t_lo <= t_hi",
                                             "has a length or a number of valid outputs that its ratio does not give",
                                             "writes outside the output buffer", "reads samples its ring does not hold"};
        sos_set_error("%s: row %d %s (slot %lld of %lld, outputs %lld .. %lld, n_in %lld, n_valid %lld, output offset %lld of %lld, "
                      "a ring of %lld samples, a wing of %lld)", who, r, reason[why], (long long)e.slot, (long long)slots,
                      (long long)e.t_lo, (long long)e.t_hi, (long long)e.n_in, (long long)e.n_valid, (long long)e.out_off,
                      (long long)total, (long long)cap, (long long)f.reach);
        return SOS_EINVAL;
    }
    if (total_tiles == 0) return SOS_OK;              // every row is empty
    const unsigned grid = rs_grid(who, total_tiles);
    if (!grid) return SOS_ELAUNCH;
    return rs_launch<stream_resample_kernel>(who, grid, SRS_THREADS, f.lds, stream, ring, slots, cap, table, nrows, total, max_t, ratio,
                                             seg, f.scale, win, nwin, num_table, f.index_step, tile, out);
}
