// band_merge.hip -- the band above 7 kHz of a recording whose rate exceeds the networks' 14 kHz (recordings.denoise_recordings,
// high_band='keep' / 'follow').  Per channel: x = the native plane (n frames), a = x at 14 kHz (m samples, what the networks
// saw), b = their output (m' = hop * (m // hop) samples), U = sos_resample_f32 back to the native rate.  Today's output is
// U(b); what the 14 kHz chain never saw is x - U(a), and
//     out[t] = fmaf(g[t], x[t] - U(a)[t], U(b)[t])        0 <= t < n, all f32
// puts it back: g = 1 ('keep'), or the attenuation the networks applied to the low band, frame by frame ('follow').
//   sos_band_gain_batch_f32       s[j] per hop frame of a ragged batch: energies, ratio, clip, smoothing
//   sos_resample_merge_batch_f32  the rule above for a ragged batch at one ratio, one launch: both resamplings (rs_output2 of
//                                 resample_core.h: the bits of rs_output, each tap weight formed once), g[t] interpolated from s
// Float64 restatement: tests/band_reference.py.
#include "band_core.h"
#include "resample_launch.h"

#define BM_THREADS 1024         // the merge kernel's workgroup, as the batch resampler's (wave_io.hip)
#define BM_PER_WG 4096          // = SOS_RESAMPLE_CHUNK
#define BG_TILE 64              // frames of s per workgroup pass of the gain kernel
// BG_MAX_SMOOTH (band_core.h), K <= 16: a tile of r plus K frames of halo on each side lives in LDS
#define BG_MAX_GRID_X 64

// ---------------------------------------------------------------------------------------------- gains
// Table int64 [6][nclips]: [0] a offset [1] m [2] b offset [3] m' [4] gains offset [5] J = ceil(m / hop).
// Frame j covers the low-rate samples [j hop, (j + 1) hop) cut at m; E_a = sum a^2, E_b = sum b^2 (b reads zero from m' on),
// both in f64; r[j] = 1 if E_a == 0 else min(1, sqrt(E_b / E_a)); s[j] = the f64 mean of r[max(0, j - K) .. min(J - 1, j + K)],
// stored as f32.  grid (x, clip): the workgroups of a clip walk its tiles of BG_TILE frames, one wave per frame of r.
struct BandGainClip { int64_t a_off, m, b_off, mp, g_off, J; };
__host__ __device__ static inline BandGainClip band_gain_row(const int64_t* tab, int64_t nclips, int64_t c) {
    return {tab[c], tab[nclips + c], tab[2 * nclips + c], tab[3 * nclips + c], tab[4 * nclips + c], tab[5 * nclips + c]};
}
// Why a clip cannot be followed (0: it can): the rule of ragged.h against the totals the host summed from its own table, for
// the kernel's skip and the host's refusal alike
enum { BM_OK = 0, BM_COUNTS, BM_A, BM_B, BM_GAINS, BM_ROW };
__host__ __device__ static inline int band_gain_why(const BandGainClip& e, int64_t total_a, int64_t total_b, int64_t total_g, int hop) {
    if (e.m < 1 || e.mp < 0 || e.mp > e.m) return BM_COUNTS;
    if (!ragged_clip_inside(e.a_off, e.m, total_a)) return BM_A;
    if (!ragged_clip_inside(e.b_off, e.mp, total_b)) return BM_B;
    if (e.J != (e.m - 1) / hop + 1 || !ragged_clip_inside(e.g_off, e.J, total_g)) return BM_GAINS;
    return BM_OK;
}
__global__ __launch_bounds__(MT) void band_gain_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const int64_t* __restrict__ tab, int nclips, int64_t total_a, int64_t total_b,
                                                       int64_t total_g, int hop, int K, float* __restrict__ gains) {
    __shared__ double r[BG_TILE + 2 * BG_MAX_SMOOTH];
    const BandGainClip e = band_gain_row(tab, nclips, blockIdx.y);
    if (band_gain_why(e, total_a, total_b, total_g, hop) != BM_OK) return;      // a device row the host did not size: no work
    const int64_t m = e.m, mp = e.mp, J = e.J;
    const float* ac = a + e.a_off;
    const float* bc = b + e.b_off;
    float* gc = gains + e.g_off;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t j0 = (int64_t)blockIdx.x * BG_TILE; j0 < J; j0 += (int64_t)gridDim.x * BG_TILE) {
        const int64_t lo = j0 - K > 0 ? j0 - K : 0;
        const int64_t hi = j0 + BG_TILE + K < J ? j0 + BG_TILE + K : J;
        for (int64_t j = lo + wave; j < hi; j += MT / 64) {
            const int64_t s0 = j * hop, s1 = s0 + hop < m ? s0 + hop : m;
            const double rj = band_frame_ratio(RsLinear{ac}, RsLinear{bc}, s0, s1, mp, lane);
            if (lane == 0) r[j - lo] = rj;
        }
        __syncthreads();
        for (int64_t j = j0 + threadIdx.x; j < j0 + BG_TILE && j < J; j += MT) gc[j] = band_mean(BandRTile{r, lo}, j, K, J);
        __syncthreads();
    }
}

extern "C" int sos_band_gain_batch_f32(const float* a, const float* b, const int64_t* table, const int64_t* table_host, int nclips,
                                       int hop, int smooth, float* gains, sos_stream_t stream) {
    const char* who = "sos_band_gain_batch_f32";
    if (!a || !b || !table || !table_host || !gains) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (nclips < 1 || nclips > RAGGED_MAX_CLIPS || hop < 1 || smooth < 0 || smooth > BG_MAX_SMOOTH) {
        sos_set_error("%s: bad args (1 .. 65535 clips, got %d; hop=%d: at least 1; smooth=%d: 0 .. %d frames)", who, nclips, hop, smooth,
                      BG_MAX_SMOOTH);
        return SOS_EINVAL;
    }
    int64_t total_a = 0, total_b = 0, total_g = 0, max_J = 0;
    for (int c = 0; c < nclips; ++c) {
        const BandGainClip e = band_gain_row(table_host, nclips, c);
        if (e.m < 1 || e.m > (int64_t)1 << 52 || e.mp < 0 || e.mp > e.m) {
            sos_set_error("%s: clip %d has m=%lld, m'=%lld (m at least 1, m' within 0 .. m)", who, c, (long long)e.m, (long long)e.mp);
            return SOS_EINVAL;
        }
        const int64_t want = (e.m - 1) / hop + 1;
        if (e.J != want) {
            sos_set_error("%s: clip %d has %lld frames (m=%lld, hop=%d: %lld expected)", who, c, (long long)e.J, (long long)e.m, hop,
                          (long long)want);
            return SOS_EINVAL;
        }
        if (e.a_off < total_a || e.b_off < total_b || e.g_off < total_g || e.a_off > INT64_MAX / 8 || e.b_off > INT64_MAX / 8 ||
            e.g_off > INT64_MAX / 8) {
            sos_set_error("%s: clip %d overlaps its predecessor or is out of order (a %lld, b %lld, gains %lld)", who, c,
                          (long long)e.a_off, (long long)e.b_off, (long long)e.g_off);
            return SOS_EINVAL;
        }
        total_a = e.a_off + e.m;
        total_b = e.b_off + e.mp;
        total_g = e.g_off + e.J;
        max_J = std::max(max_J, e.J);
    }
    for (int c = 0; c < nclips; ++c)                             // what the kernel will ask of each clip
        if (const int why = band_gain_why(band_gain_row(table_host, nclips, c), total_a, total_b, total_g, hop)) {
            sos_set_error("%s: clip %d lies outside the totals of the table (rule %d)", who, c, why);
            return SOS_EINVAL;
        }
    const dim3 grid(ragged_grid(max_J, BG_TILE, BG_MAX_GRID_X), (unsigned)nclips);
    hipLaunchKernelGGL(band_gain_kernel, grid, dim3(MT), 0, (hipStream_t)stream, a, b, table, nclips, total_a, total_b, total_g, hop,
                       smooth, gains);
    return sos_check_launch(who);
}

// ---------------------------------------------------------------------------------------------- merge
// Table int64 [9][nclips]: [0] offset of the clip in x AND in out [1] n [2] a offset [3] m [4] b offset [5] m' [6] gains offset
// [7] J [8] the clip's first tile = sum of ceil(n / BM_PER_WG) over the clips before it.  The structure of
// resample_batch_kernel (wave_io.hip): one workgroup per CU loads the window once and walks the (clip, BM_PER_WG outputs) tiles.
// g[t] = linear interpolation of s at the frame-centre position p = (t + 0.5) / (ratio hop) - 0.5, clamped to s[0] for p <= 0
// and to s[J - 1] for p >= J - 1, evaluated in f64 and rounded to f32; gains == NULL: g = 1.
struct BandMergeClip { int64_t x_off, n, a_off, m, b_off, mp, g_off, J, tile0; };
__host__ __device__ static inline BandMergeClip band_merge_row(const int64_t* tab, int64_t nclips, int64_t c) {
    return {tab[c], tab[nclips + c], tab[2 * nclips + c], tab[3 * nclips + c], tab[4 * nclips + c], tab[5 * nclips + c],
            tab[6 * nclips + c], tab[7 * nclips + c], tab[8 * nclips + c]};
}
// Why `tile` of a clip cannot be followed (0: it can).  max_n: the outputs the time register describes; with_gains: whether
// the gains columns count.  The row by value and ONE test of it, as the kernel had: a chain of tests with a code each, or the
// row by reference, costs resample_merge_kernel scalar registers it does not have (EXPERIMENTS.md 3.30).
__host__ __device__ static inline int band_merge_why(const BandMergeClip e, int64_t total_x, int64_t total_a, int64_t total_b,
                                                     int64_t total_g, int64_t max_n, double ratio, int hop, bool with_gains,
                                                     int64_t tile) {
    const int64_t t0 = (tile - e.tile0) * BM_PER_WG;
    if (e.n < 1 || e.n > max_n || e.m < 1 || e.m > ((int64_t)1 << 52) || e.mp < 1 || e.mp > e.m ||
        !ragged_clip_inside(e.x_off, e.n, total_x) || !ragged_clip_inside(e.a_off, e.m, total_a) ||
        !ragged_clip_inside(e.b_off, e.mp, total_b) || t0 < 0 || t0 >= e.n || (int64_t)((double)e.m * ratio) < e.n)
        return BM_ROW;                                                // the last: a does not cover the clip
    if (with_gains && (e.J != (e.m - 1) / hop + 1 || !ragged_clip_inside(e.g_off, e.J, total_g))) return BM_GAINS;
    return BM_OK;
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void resample_merge_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                                 const float* __restrict__ b, const float* __restrict__ gains,
                                                                 const int64_t* __restrict__ tab, int nclips, int64_t total_x,
                                                                 int64_t total_a, int64_t total_b, int64_t total_g, int64_t total_tiles,
                                                                 int64_t max_n, RsSegs seg, double ratio, double scale,
                                                                 const float* __restrict__ win, int nwin, int num_table, int index_step,
                                                                 int hop, float* __restrict__ out) {
    extern __shared__ float w[];
    rs_load_window<THREADS>(w, win, nwin);
    const double frame = ratio * (double)hop;                     // native frames per hop of the low rate
    for (int64_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const BandMergeClip e = band_merge_row(tab, nclips, rs_clip_of_tile(tab + 8 * (int64_t)nclips, nclips, tile));
        if (band_merge_why(e, total_x, total_a, total_b, total_g, max_n, ratio, hop, gains != nullptr, tile) != BM_OK) continue;
        const int64_t t0 = (tile - e.tile0) * BM_PER_WG, n = e.n, m = e.m, mp = e.mp, J = e.J;
        const int64_t vb = (int64_t)((double)mp * ratio);     // U(b) is resampled below vb and zero from there on
        const float* xc = x + e.x_off;
        const float* ac = a + e.a_off;
        const float* bc = b + e.b_off;
        const float* sc = gains ? gains + e.g_off : nullptr;
        float* oc = out + e.x_off;
        for (int64_t t = t0 + threadIdx.x; t < t0 + BM_PER_WG && t < n; t += THREADS) {
            float ra, rb;
            rs_output2(RsLinear{ac}, m, RsLinear{bc}, mp, t < vb, seg, scale, w, nwin, num_table, index_step, t, &ra, &rb);
            const float g = sc ? band_gain_at([sc](int64_t j) { return sc[j]; }, band_gain_pos(t, frame), J) : 1.f;
            const float h = xc[t] - ra;
            oc[t] = fmaf(g, h, rb);
        }
    }
}

extern "C" int sos_resample_merge_batch_f32(const float* x, const float* a, const float* b, const float* gains, const int64_t* table,
                                            const int64_t* table_host, int nclips, double ratio, const float* win, int nwin,
                                            int num_table, int hop, float* out, sos_stream_t stream) {
    const char* who = "sos_resample_merge_batch_f32";
    if (!x || !a || !b || !table || !table_host || !win || !out) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (nclips < 1 || nclips > RAGGED_MAX_CLIPS || hop < 1) {
        sos_set_error("%s: bad args (1 .. 65535 clips, got %d; hop=%d: at least 1)", who, nclips, hop);
        return SOS_EINVAL;
    }
    RsFilter f;
    if (!rs_filter(who, ratio, nwin, num_table, true, &f)) return SOS_EINVAL;
    int64_t total_x = 0, total_a = 0, total_b = 0, total_g = 0, total_tiles = 0, max_n = 0;
    for (int c = 0; c < nclips; ++c) {
        const BandMergeClip e = band_merge_row(table_host, nclips, c);
        if (e.n < 1 || e.n > (int64_t)1 << 52 || e.m < 1 || e.m > (int64_t)1 << 52 || e.mp < 1 || e.mp > e.m) {
            sos_set_error("%s: clip %d has n=%lld, m=%lld, m'=%lld (each at least 1, m' at most m)", who, c, (long long)e.n,
                          (long long)e.m, (long long)e.mp);
            return SOS_EINVAL;
        }
        const int64_t covered = (int64_t)((double)e.m * ratio);      // resampy's output length for a, as sos_resample_f32 computes it
        if (covered < e.n) {
            sos_set_error("%s: clip %d has n=%lld frames but its m=%lld low-rate samples cover %lld at ratio %g", who, c,
                          (long long)e.n, (long long)e.m, (long long)covered, ratio);
            return SOS_EINVAL;
        }
        if (gains && e.J != (e.m - 1) / hop + 1) {
            sos_set_error("%s: clip %d has %lld gains (m=%lld, hop=%d: %lld expected)", who, c, (long long)e.J, (long long)e.m, hop,
                          (long long)((e.m - 1) / hop + 1));
            return SOS_EINVAL;
        }
        if (e.x_off < total_x || e.a_off < total_a || e.b_off < total_b || (gains && e.g_off < total_g) || e.tile0 != total_tiles ||
            e.x_off > INT64_MAX / 8 || e.a_off > INT64_MAX / 8 || e.b_off > INT64_MAX / 8 || (gains && e.g_off > INT64_MAX / 8)) {
            sos_set_error("%s: clip %d overlaps its predecessor or is out of order (x %lld, a %lld, b %lld, gains %lld, first tile %lld "
                          "where %lld is expected)", who, c, (long long)e.x_off, (long long)e.a_off, (long long)e.b_off,
                          (long long)e.g_off, (long long)e.tile0, (long long)total_tiles);
            return SOS_EINVAL;
        }
        total_x = e.x_off + e.n;
        total_a = e.a_off + e.m;
        total_b = e.b_off + e.mp;
        if (gains) total_g = e.g_off + e.J;
        total_tiles += (e.n + BM_PER_WG - 1) / BM_PER_WG;
        max_n = std::max(max_n, e.n);
    }
    for (int c = 0; c < nclips; ++c) {                           // what the kernel will ask of each clip, first tile and last
        const BandMergeClip e = band_merge_row(table_host, nclips, c);
        for (const int64_t tile : {e.tile0, e.tile0 + (e.n - 1) / BM_PER_WG})
            if (const int why = band_merge_why(e, total_x, total_a, total_b, total_g, max_n, ratio, hop, gains != nullptr, tile)) {
                sos_set_error("%s: clip %d lies outside the totals of the table (rule %d, tile %lld)", who, c, why, (long long)tile);
                return SOS_EINVAL;
            }
    }
    RsSegs seg;
    if (const int rc = rs_segments(who, ratio, max_n, &seg)) return rc;
    const unsigned grid = rs_grid(who, total_tiles);
    if (!grid) return SOS_ELAUNCH;
    return rs_launch<resample_merge_kernel<BM_THREADS>>(who, grid, BM_THREADS, f.lds, stream, x, a, b, gains, table, nclips, total_x,
                                                        total_a, total_b, total_g, total_tiles, max_n, seg, ratio, f.scale, win, nwin,
                                                        num_table, f.index_step, hop, out);
}
