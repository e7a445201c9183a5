// loudness_core.h -- what the entry points on the loudness table share (loudness.hip: the measurement, the gain, the true peak and
// the range; limiter.hip: the look-ahead limiter): the table's row rule on both sides of the launch, the host's checks of a
// table, and the one interpolated point of the true peak.
#pragma once
#include "ragged.h"

#define LD_COLS 8                       // int64 per file: the encode row {first plane sample, plane length, channels, frames, H of the
                                        // limiter (read by limiter.hip only)}, then {hop h, first channel weight, first chunk of the work arrays}
#define LD_WAVE 64                      // threads per workgroup of the chunk kernels: 64 consecutive chunks of one plane
#define LD_MAX_CHANNELS 64
#define LD_MAX_SPLIT 64
#define LD_MAX_HOP ((int64_t)1 << 31)

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

// The true peak's interpolated point n + p / 4: v = sum_k h_p[k] x[n + k] for the taps k = -5 .. 6, 12 fmaf in tap order in
// float32; w[0 .. 12) = x[n - 5 .. n + 6].
#define TP_TAPS 12
__device__ __forceinline__ float tp_point(const float (&h)[TP_TAPS], const float* w) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < TP_TAPS; ++k) v = fmaf(h[k], w[k], v);
    return v;
}
