// stream_band.hip -- the band above 7 kHz of LIVE audio whose rate exceeds the networks' 14 kHz (audio_io.StreamBandMerger,
// stream.StreamDenoiser(high_band='keep' / 'follow')): band_merge.hip's rule for streams that arrive in chunks.  With x the
// native stream, a = x at 14 kHz, b = the networks' output and U the resampling back (an upsampling: scale = 1, index_step =
// num_table, R = nwin / num_table samples per wing)
//     out[t] = fmaf(g[t], x[t] - U(a)[t], U(b)[t])
// with the bits of sos_resample_merge_batch_f32 for the whole signals, whatever the chunking: both resamplings by rs_output2
// (resample_core.h), the gains by the functions of band_core.h that the file kernels call.
// Finality (float64 / integer restatement: tests/stream_band_reference.py).  With n_x native samples and m_b final samples of b
// received (a never trails b), output t has the bits it has for any longer stream once
//     n(t) + 1 + R <= m_b                       neither right wing is cut (sos_stream_resample_ready at the ratio, asked about m_b)
//     band_gain_last(p(t)) < m_b / hop - K      'follow': g[t] reads s up to that frame, s[j] is final once r[j + K] is, r[j]
//                                               once (j + 1) hop <= m_b -- then no end clamps p and none cuts the mean
//     t < n_x                                   x[t] has arrived
// All three hold for a prefix of t, T = its length.  Later outputs read x from T, a and b from max(n(T) - (R - 1), 0) -- under
// 'follow' also from hop * (m_b / hop), the first sample of a frame without r -- and r from max(band_gain_last(p(T)) - 1 - K, 0).
// State, on the device: ring f32 [3 slots][cap], row slot = x, slots + slot = a, 2 slots + slot = b of a stream, sample p at
// [p % cap] (sos_stream_push_f32 fills all three in one launch); rring f64 [slots][rcap], frame j of r at [j % rcap].
//   sos_stream_band_ready       host only: T and the first retained x, a, b sample and r frame, from the expressions the kernels
//                               evaluate (rs_time, band_gain_pos): a count off by one would emit a sample that is not final
//   sos_stream_band_ratio_f64   one launch for all slots: row = (slot, frames [j_lo, j_hi), m_a, m_b) -> r[j] into the slot's
//                               ring of frames; a is cut at m_a, b reads zero from m_b on (at close: the last partial frame)
//   sos_stream_band_merge_f32   one launch for all slots, the shape of stream_resample_kernel: the window in LDS, at most one
//                               workgroup per CU, tiles of 256 outputs walked gridDim.x apart in one ascending pass over the rows
// Bounds: the rule of ragged.h as in stream_resample.hip -- the host refuses a row that leaves what the rings hold (SOS_EINVAL,
// the row is named) or names a slot twice, the kernels skip a row of the DEVICE table that fails the same test.  Ring indices
// are modular.  No atomics.
#include "band_core.h"
#include "resample_launch.h"

#define SB_THREADS 256
#define SB_TILE 256                     // outputs per workgroup step
#define SB_RATIO_COLS 5
#define SB_MERGE_COLS 10
#define SB_MAX_POS ((int64_t)1 << 52)   // stream positions: exact in f64
#define SB_MAX_HOP (1 << 20)
#define SB_RATIO_GRID_X 64

// ---------------------------------------------------------------------------------------------- r[j]
struct StreamBandRatio { int64_t slot, j_lo, j_hi, m_a, m_b; };
__host__ __device__ static inline StreamBandRatio stream_band_ratio_row(const int64_t* table, int64_t r) {
    const int64_t* te = table + r * SB_RATIO_COLS;
    return {te[0], te[1], te[2], te[3], te[4]};
}
enum { SB_OK = 0, SB_SLOT, SB_RANGE, SB_VALID, SB_OUTPUT, SB_SPAN_X, SB_SPAN, SB_FRAMES };
__host__ __device__ static inline int stream_band_ratio_why(const StreamBandRatio& e, int64_t slots, int64_t cap, int64_t rcap,
                                                            int hop) {
    if (e.slot < 0 || e.slot >= slots) return SB_SLOT;
    if (e.m_a < 0 || e.m_a > SB_MAX_POS || e.m_b < 0 || e.m_b > e.m_a) return SB_VALID;
    if (e.j_lo < 0 || e.j_lo > e.j_hi || e.j_hi - e.j_lo > rcap || e.j_hi > (e.m_a + hop - 1) / hop) return SB_RANGE;
    if (e.j_lo < e.j_hi && e.m_a - e.j_lo * hop > cap) return SB_SPAN;       // the ring holds the last `cap` samples before m_a
    return SB_OK;
}

// grid (x, row): the workgroups of a row walk its frames, one wave per frame
__global__ __launch_bounds__(MT) void stream_band_ratio_kernel(const float* __restrict__ ring, int64_t slots, int64_t cap,
                                                               const int64_t* __restrict__ table, int hop,
                                                               double* __restrict__ rring, int64_t rcap) {
    const StreamBandRatio e = stream_band_ratio_row(table, blockIdx.y);
    if (stream_band_ratio_why(e, slots, cap, rcap, hop) != SB_OK) return;      // a device row the host did not size: no work
    const RsRing sa{ring + (slots + e.slot) * cap, cap}, sb{ring + (2 * slots + e.slot) * cap, cap};
    double* rr = rring + e.slot * rcap;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t j = e.j_lo + (int64_t)blockIdx.x * (MT / 64) + wave; j < e.j_hi; j += (int64_t)gridDim.x * (MT / 64)) {
        const int64_t s0 = j * hop, s1 = s0 + hop < e.m_a ? s0 + hop : e.m_a;
        const double rj = band_frame_ratio(sa, sb, s0, s1, e.m_b, lane);
        if (lane == 0) rr[j % rcap] = rj;
    }
}

// three rings per slot (x, a, b) and the hop; false with the error set
static bool stream_band_rings(const char* who, int nrows, int64_t slots, int64_t cap, int hop) {
    if (!rs_rings(who, nrows, slots, 3, cap)) return false;
    if (hop < 1 || hop > SB_MAX_HOP) { sos_set_error("%s: hop=%d: 1 .. 2^20", who, hop); return false; }
    return true;
}

static const char* const stream_band_reason[] = {"",
                                                 "names a slot outside the slots",
                                                 "has a range that is none, or frames its ring of frames or its a does not have",
                                                 "has counts that do not fit (0 <= b <= a, valid outputs of b within its length)",
                                                 "writes outside the output buffer",
                                                 "reads native samples its ring does not hold",
                                                 "reads samples of a or b their rings do not hold",
                                                 "reads frames of r its ring of frames does not hold"};

extern "C" int sos_stream_band_ratio_f64(const float* ring, int64_t slots, int64_t cap, const int64_t* table,
                                         const int64_t* table_host, int nrows, int hop, double* rring, int64_t rcap,
                                         sos_stream_t stream) {
    const char* who = "sos_stream_band_ratio_f64";
    if (!ring || !table || !table_host || !rring) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (!stream_band_rings(who, nrows, slots, cap, hop)) return SOS_EINVAL;
    if (rcap < 1 || rcap > INT64_MAX / 8 / RAGGED_MAX_CLIPS) {
        sos_set_error("%s: a ring of %lld frames", who, (long long)rcap);
        return SOS_EINVAL;
    }
    RsSlotsOnce once(slots);
    int64_t most = 0;
    for (int r = 0; r < nrows; ++r) {
        const StreamBandRatio e = stream_band_ratio_row(table_host, r);
        const int why = stream_band_ratio_why(e, slots, cap, rcap, hop);
        if (why != SB_OK) {
            sos_set_error("%s: row %d %s (slot %lld of %lld, frames %lld .. %lld of hop %d, a %lld, b %lld, rings of %lld samples and "
                          "%lld frames)", who, r, stream_band_reason[why], (long long)e.slot, (long long)slots, (long long)e.j_lo,
                          (long long)e.j_hi, hop, (long long)e.m_a, (long long)e.m_b, (long long)cap, (long long)rcap);
            return SOS_EINVAL;
        }
        if (!once.take(who, r, e.slot)) return SOS_EINVAL;
        most = std::max(most, e.j_hi - e.j_lo);
    }
    if (most == 0) return SOS_OK;
    const dim3 grid(ragged_grid(most, MT / 64, SB_RATIO_GRID_X), (unsigned)nrows);
    hipLaunchKernelGGL(stream_band_ratio_kernel, grid, dim3(MT), 0, (hipStream_t)stream, ring, slots, cap, table, hop, rring, rcap);
    return sos_check_launch(who);
}

// ---------------------------------------------------------------------------------------------- merge
// A row: the outputs [t_lo, t_hi) of stream `slot` as of n_x native samples, n_a samples of a and n_b of b (U(b) is zero from
// output v_b on), J frames of s (-1: the stream is open, no end is known) and r_hi frames of r written so far.
struct StreamBand { int64_t slot, t_lo, t_hi, n_x, n_a, n_b, v_b, J, r_hi, out_off; };
__host__ __device__ static inline StreamBand stream_band_row(const int64_t* table, int64_t r) {
    const int64_t* te = table + r * SB_MERGE_COLS;
    return {te[0], te[1], te[2], te[3], te[4], te[5], te[6], te[7], te[8], te[9]};
}
// Why a row cannot be followed (0: it can).  K < 0: no gains.  frame = ratio * hop.
__host__ __device__ static inline int stream_band_why(const StreamBand& e, int64_t slots, int64_t cap, int64_t rcap, int64_t total,
                                                      int64_t max_t, double ratio, int64_t reach, const RsSegs& seg, int hop, int K,
                                                      double frame) {
    if (e.slot < 0 || e.slot >= slots) return SB_SLOT;
    if (e.t_lo < 0 || e.t_lo > e.t_hi || e.t_hi > max_t) return SB_RANGE;
    if (e.n_x < 0 || e.n_x > SB_MAX_POS || e.n_a < 0 || e.n_a > SB_MAX_POS || e.n_b < 0 || e.n_b > e.n_a || e.v_b < 0 ||
        e.v_b > (int64_t)((double)e.n_b * ratio))
        return SB_VALID;
    if (!ragged_clip_inside(e.out_off, e.t_hi - e.t_lo, total)) return SB_OUTPUT;
    if (e.t_lo == e.t_hi) return SB_OK;
    if (e.t_hi > e.n_x || e.n_x - e.t_lo > cap) return SB_SPAN_X;
    // a and b: read from n(t_lo) - (R - 1) on, none at or past n_a (n_b); a ring holds the last `cap` before its count
    const int64_t first = (int64_t)rs_time(seg, e.t_lo) - (reach - 1), last = (int64_t)rs_time(seg, e.t_hi - 1);
    if (last >= e.n_a || e.n_a - (first > 0 ? first : 0) > cap) return SB_SPAN;
    if (K >= 0) {
        if (e.r_hi < 0 || e.r_hi > SB_MAX_POS) return SB_FRAMES;
        const double p_lo = band_gain_pos(e.t_lo, frame), p_hi = band_gain_pos(e.t_hi - 1, frame);
        int64_t i_lo = band_gain_last(p_lo) - 1;                 // the first frame of s read: floor(p), 0 for p <= 0
        if (i_lo < 0) i_lo = 0;
        if (e.J < 0) {
            if (band_gain_last(p_hi) + K >= e.r_hi) return SB_FRAMES;       // s up to that frame, each r up to K further
        } else {
            if (e.n_a < 1 || e.J != (e.n_a - 1) / hop + 1 || e.r_hi != e.J) return SB_FRAMES;
            if (i_lo > e.J - 1) i_lo = e.J - 1;
        }
        if (e.r_hi - (i_lo - K > 0 ? i_lo - K : 0) > rcap) return SB_FRAMES;
    }
    return SB_OK;
}
__host__ __device__ static inline int64_t stream_band_tiles(const StreamBand& e) { return (e.t_hi - e.t_lo + SB_TILE - 1) / SB_TILE; }

__global__ __launch_bounds__(SB_THREADS) void stream_band_merge_kernel(const float* __restrict__ ring, int64_t slots, int64_t cap,
                                                                       const double* __restrict__ rring, int64_t rcap,
                                                                       const int64_t* __restrict__ table, int nrows, int64_t total,
                                                                       int64_t max_t, double ratio, RsSegs seg,
                                                                       const float* __restrict__ win, int nwin, int num_table,
                                                                       int hop, int K, float* __restrict__ out) {
    extern __shared__ float w[];
    rs_load_window<SB_THREADS>(w, win, nwin);
    const int index_step = num_table;                            // an upsampling: scale = 1
    const int64_t reach = nwin / index_step;
    const double frame = ratio * (double)hop;
    // the tiles of the rows lie back to back in table order; this workgroup's tiles ascend, so one pass over the rows serves all
    // (the walk of stream_resample_kernel; a shared form of it changed this kernel's code and its time, EXPERIMENTS.md 3.30)
    int r = 0;
    bool read = false;
    int64_t tile0 = 0, tiles = 0;
    StreamBand e = {};
    for (int64_t tile = blockIdx.x;; tile += gridDim.x) {
        for (; r < nrows; tile0 += tiles, ++r, read = false) {
            if (!read) {
                e = stream_band_row(table, r);
                tiles = stream_band_why(e, slots, cap, rcap, total, max_t, ratio, reach, seg, hop, K, frame) == SB_OK
                            ? stream_band_tiles(e) : 0;
                read = true;
            }
            if (tile < tile0 + tiles) break;
        }
        if (r == nrows) return;
        const int64_t t = e.t_lo + (tile - tile0) * SB_TILE + threadIdx.x;
        if (t < e.t_hi) {
            float ra, rb;
            rs_output2(RsRing{ring + (slots + e.slot) * cap, cap}, e.n_a, RsRing{ring + (2 * slots + e.slot) * cap, cap}, e.n_b,
                       t < e.v_b, seg, 1.0, w, nwin, num_table, index_step, t, &ra, &rb);
            float g = 1.f;
            if (K >= 0) {
                const BandRRing rr{rring + e.slot * rcap, rcap};
                const int64_t J = e.J;
                g = band_gain_at([rr, K, J](int64_t j) { return band_mean(rr, j, K, J); }, band_gain_pos(t, frame), J);
            }
            const float h = ring[e.slot * cap + t % cap] - ra;
            out[e.out_off + (t - e.t_lo)] = fmaf(g, h, rb);
        }
    }
}

// the filter of an upsampling: the rule of every resampler, a ratio within (1, 1024] and a wing of at least one sample; false
// with the error set otherwise.  launch: as rs_filter's.
static bool stream_band_filter(const char* who, double ratio, int nwin, int num_table, bool launch, RsFilter* f) {
    // the ratio first: a downsampling is told that it is one, not that its ratio is too small for the table; a bad ratio of any
    // other kind, nwin and num_table are rs_filter's.  nwin < 2 is refused for the host-only count too, as it always was here.
    const bool down = ratio > 0.0 && !(ratio > 1.0 && ratio <= 1024.0);
    if (!down && !rs_filter(who, ratio, nwin, num_table, launch, f)) return false;
    if (down || nwin < 2 || f->reach < 1) {
        sos_set_error("%s: bad args (ratio=%g: above 1, the native rate over the low one; nwin=%d, num_table=%d: a wing of at least "
                      "one sample)", who, ratio, nwin, num_table);
        return false;
    }
    return true;
}

extern "C" int sos_stream_band_ready(double ratio, int nwin, int num_table, int hop, int smooth, int64_t m_b, int64_t n_x,
                                     int64_t* t_ready, int64_t* first_x, int64_t* first_a, int64_t* first_b, int64_t* first_r) {
    const char* who = "sos_stream_band_ready";
    if (!t_ready || !first_x || !first_a || !first_b || !first_r) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    RsFilter f;
    if (!stream_band_filter(who, ratio, nwin, num_table, false, &f)) return SOS_EINVAL;
    if (hop < 1 || hop > SB_MAX_HOP || smooth > BG_MAX_SMOOTH) {
        sos_set_error("%s: hop=%d: 1 .. 2^20; smooth=%d: 0 .. %d frames, negative for no gains", who, hop, smooth, BG_MAX_SMOOTH);
        return SOS_EINVAL;
    }
    if (m_b < 0 || m_b > SB_MAX_POS || n_x < 0 || n_x > SB_MAX_POS) {
        sos_set_error("%s: a stream of %lld low-rate and %lld native samples", who, (long long)m_b, (long long)n_x);
        return SOS_EINVAL;
    }
    const int64_t reach = f.reach;
    int64_t T = 0, base = 0;
    const int rc = sos_stream_resample_ready(ratio, nwin, num_table, m_b, &T, &base);       // n(t) + 1 + R <= m_b
    if (rc != SOS_OK) return rc;
    if (n_x < T) T = n_x;                                                                  // x[t] has arrived
    const double frame = ratio * (double)hop;
    if (smooth >= 0) {
        const int64_t final_s = m_b / hop - smooth;              // s[j] is final for j below this
        if (final_s < 1) {
            T = 0;
        } else if (band_gain_last(band_gain_pos(T, frame)) >= final_s) {
            // the frame read grows with t: T = the first t that reads frame final_s or a later one
            int64_t lo = -1, hi = T;
            while (hi - lo > 1) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (band_gain_last(band_gain_pos(mid, frame)) < final_s) lo = mid; else hi = mid;
            }
            T = hi;
        }
    }
    RsSegs g;
    if (const int rc = rs_segments(who, ratio, T + 1, &g)) return rc;
    int64_t first = (int64_t)rs_time(g, T) - (reach - 1);
    if (first < 0) first = 0;
    *first_r = 0;
    if (smooth >= 0) {
        const int64_t whole = hop * (m_b / hop);                  // the first sample of a frame that has no r yet
        if (whole < first) first = whole;
        const int64_t i_lo = band_gain_last(band_gain_pos(T, frame)) - 1 - smooth;
        *first_r = i_lo > 0 ? i_lo : 0;
    }
    *t_ready = *first_x = T;
    *first_a = *first_b = first;
    return SOS_OK;
}

extern "C" int sos_stream_band_merge_f32(const float* ring, int64_t slots, int64_t cap, const double* rring, int64_t rcap,
                                         const int64_t* table, const int64_t* table_host, int nrows, double ratio, const float* win,
                                         int nwin, int num_table, int hop, int smooth, float* out, int64_t total,
                                         sos_stream_t stream) {
    const char* who = "sos_stream_band_merge_f32";
    if (!ring || !table || !table_host || !win || !out || (smooth >= 0 && !rring)) {
        sos_set_error("%s: null pointer", who);
        return SOS_EINVAL;
    }
    if (!stream_band_rings(who, nrows, slots, cap, hop)) return SOS_EINVAL;
    RsFilter f;
    if (!stream_band_filter(who, ratio, nwin, num_table, true, &f)) return SOS_EINVAL;
    if (smooth > BG_MAX_SMOOTH || (smooth >= 0 && (rcap < 1 || rcap > INT64_MAX / 8 / RAGGED_MAX_CLIPS)) || total < 0 ||
        total > INT64_MAX / 8) {
        sos_set_error("%s: bad args (smooth=%d: 0 .. %d frames, negative for no gains; a ring of %lld frames; an output of %lld)", who,
                      smooth, BG_MAX_SMOOTH, (long long)rcap, (long long)total);
        return SOS_EINVAL;
    }
    const int K = smooth < 0 ? -1 : smooth;
    const int64_t reach = f.reach;
    const double frame = ratio * (double)hop;
    RsSegs seg;
    int64_t max_t;
    const auto t_hi = [table_host](int r) { return stream_band_row(table_host, r).t_hi; };
    if (const int rc = rs_row_segments(who, nrows, t_hi, ratio, &seg, &max_t)) return rc;
    RsSlotsOnce once(slots);
    int64_t total_tiles = 0;
    for (int r = 0; r < nrows; ++r) {
        const StreamBand e = stream_band_row(table_host, r);
        const int why = stream_band_why(e, slots, cap, rcap, total, max_t, ratio, reach, seg, hop, K, frame);
        if (why != SB_OK) {
            sos_set_error("%s: row %d %s (slot %lld of %lld, outputs %lld .. %lld, x %lld, a %lld, b %lld with %lld valid outputs, "
                          "J %lld, %lld frames of r, output offset %lld of %lld, rings of %lld samples and %lld frames, a wing of "
                          "%lld)", who, r, stream_band_reason[why], (long long)e.slot, (long long)slots, (long long)e.t_lo,
                          (long long)e.t_hi, (long long)e.n_x, (long long)e.n_a, (long long)e.n_b, (long long)e.v_b, (long long)e.J,
                          (long long)e.r_hi, (long long)e.out_off, (long long)total, (long long)cap, (long long)rcap,
                          (long long)reach);
            return SOS_EINVAL;
        }
        if (!once.take(who, r, e.slot)) return SOS_EINVAL;
        total_tiles += stream_band_tiles(e);
    }
    if (total_tiles == 0) return SOS_OK;              // every row is empty
    const unsigned grid = rs_grid(who, total_tiles);
    if (!grid) return SOS_ELAUNCH;
    return rs_launch<stream_band_merge_kernel>(who, grid, SB_THREADS, f.lds, stream, ring, slots, cap, rring, rcap, table, nrows, total,
                                               max_t, ratio, seg, win, nwin, num_table, hop, K, out);
}
