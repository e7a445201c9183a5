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
__global__ __launch_bounds__(MT) void band_gain_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const int64_t* __restrict__ tab, int nclips, int64_t total_a, int64_t total_b,
                                                       int64_t total_g, int hop, int K, float* __restrict__ gains) {
    __shared__ double r[BG_TILE + 2 * BG_MAX_SMOOTH];
    const int c = blockIdx.y;
    const int64_t a_off = tab[c], m = tab[nclips + c], b_off = tab[2 * (int64_t)nclips + c], mp = tab[3 * (int64_t)nclips + c];
    const int64_t g_off = tab[4 * (int64_t)nclips + c], J = tab[5 * (int64_t)nclips + c];
    if (m < 1 || mp < 0 || mp > m || !ragged_clip_inside(a_off, m, total_a) || !ragged_clip_inside(b_off, mp, total_b) ||
        J != (m - 1) / hop + 1 || !ragged_clip_inside(g_off, J, total_g))
        return;                                                  // a device row the host did not size: no work
    const float* ac = a + a_off;
    const float* bc = b + b_off;
    float* gc = gains + g_off;
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
    if (!a || !b || !table || !table_host || !gains) { sos_set_error("sos_band_gain_batch_f32: null pointer"); return SOS_EINVAL; }
    if (nclips < 1 || nclips > RAGGED_MAX_CLIPS || hop < 1 || smooth < 0 || smooth > BG_MAX_SMOOTH) {
        sos_set_error("sos_band_gain_batch_f32: bad args (1 .. 65535 clips, got %d; hop=%d: at least 1; smooth=%d: 0 .. %d frames)",
                      nclips, hop, smooth, BG_MAX_SMOOTH);
        return SOS_EINVAL;
    }
    const int64_t *a_off = table_host, *m = a_off + nclips, *b_off = m + nclips, *mp = b_off + nclips, *g_off = mp + nclips,
                  *J = g_off + nclips;
    int64_t total_a = 0, total_b = 0, total_g = 0, max_J = 0;
    for (int c = 0; c < nclips; ++c) {
        if (m[c] < 1 || m[c] > (int64_t)1 << 52 || mp[c] < 0 || mp[c] > m[c]) {
            sos_set_error("sos_band_gain_batch_f32: clip %d has m=%lld, m'=%lld (m at least 1, m' within 0 .. m)", c, (long long)m[c],
                          (long long)mp[c]);
            return SOS_EINVAL;
        }
        const int64_t want = (m[c] - 1) / hop + 1;
        if (J[c] != want) {
            sos_set_error("sos_band_gain_batch_f32: clip %d has %lld frames (m=%lld, hop=%d: %lld expected)", c, (long long)J[c],
                          (long long)m[c], hop, (long long)want);
            return SOS_EINVAL;
        }
        if (a_off[c] < total_a || b_off[c] < total_b || g_off[c] < total_g || a_off[c] > INT64_MAX / 8 || b_off[c] > INT64_MAX / 8 ||
            g_off[c] > INT64_MAX / 8) {
            sos_set_error("sos_band_gain_batch_f32: clip %d overlaps its predecessor or is out of order (a %lld, b %lld, gains %lld)",
                          c, (long long)a_off[c], (long long)b_off[c], (long long)g_off[c]);
            return SOS_EINVAL;
        }
        total_a = a_off[c] + m[c];
        total_b = b_off[c] + mp[c];
        total_g = g_off[c] + J[c];
        max_J = std::max(max_J, J[c]);
    }
    const dim3 grid(ragged_grid(max_J, BG_TILE, BG_MAX_GRID_X), (unsigned)nclips);
    hipLaunchKernelGGL(band_gain_kernel, grid, dim3(MT), 0, (hipStream_t)stream, a, b, table, nclips, total_a, total_b, total_g, hop,
                       smooth, gains);
    return sos_check_launch("sos_band_gain_batch_f32");
}

// ---------------------------------------------------------------------------------------------- merge
// Table int64 [9][nclips]: [0] offset of the clip in x AND in out [1] n [2] a offset [3] m [4] b offset [5] m' [6] gains offset
// [7] J [8] the clip's first tile = sum of ceil(n / BM_PER_WG) over the clips before it.  The structure of
// resample_batch_kernel (wave_io.hip): one workgroup per CU loads the window once and walks the (clip, BM_PER_WG outputs) tiles.
// g[t] = linear interpolation of s at the frame-centre position p = (t + 0.5) / (ratio hop) - 0.5, clamped to s[0] for p <= 0
// and to s[J - 1] for p >= J - 1, evaluated in f64 and rounded to f32; gains == NULL: g = 1.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void resample_merge_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                                 const float* __restrict__ b, const float* __restrict__ gains,
                                                                 const int64_t* __restrict__ tab, int nclips, int64_t total_x,
                                                                 int64_t total_a, int64_t total_b, int64_t total_g, int64_t total_tiles,
                                                                 int64_t max_n, RsSegs seg, double ratio, double scale,
                                                                 const float* __restrict__ win, int nwin, int num_table, int index_step,
                                                                 int hop, float* __restrict__ out) {
    extern __shared__ float w[];
    for (int i = threadIdx.x; i <= nwin; i += THREADS) w[i] = win[i < nwin ? i : nwin - 1];
    __syncthreads();
    const int64_t* tile0 = tab + 8 * (int64_t)nclips;
    const double frame = ratio * (double)hop;                     // native frames per hop of the low rate
    for (int64_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        int lo = 0, hi = nclips - 1;                          // the last clip whose first tile is <= tile
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tile0[mid] <= tile) lo = mid; else hi = mid - 1;
        }
        const int64_t x_off = tab[lo], n = tab[nclips + lo], a_off = tab[2 * (int64_t)nclips + lo], m = tab[3 * (int64_t)nclips + lo];
        const int64_t b_off = tab[4 * (int64_t)nclips + lo], mp = tab[5 * (int64_t)nclips + lo];
        const int64_t g_off = tab[6 * (int64_t)nclips + lo], J = tab[7 * (int64_t)nclips + lo];
        const int64_t t0 = (tile - tile0[lo]) * BM_PER_WG;
        if (n < 1 || n > max_n || m < 1 || m > ((int64_t)1 << 52) || mp < 1 || mp > m || !ragged_clip_inside(x_off, n, total_x) ||
            !ragged_clip_inside(a_off, m, total_a) || !ragged_clip_inside(b_off, mp, total_b) || t0 < 0 || t0 >= n ||
            (int64_t)((double)m * ratio) < n)
            continue;
        if (gains && (J != (m - 1) / hop + 1 || !ragged_clip_inside(g_off, J, total_g))) continue;
        const int64_t vb = (int64_t)((double)mp * ratio);     // U(b) is resampled below vb and zero from there on
        const float* xc = x + x_off;
        const float* ac = a + a_off;
        const float* bc = b + b_off;
        const float* sc = gains ? gains + g_off : nullptr;
        float* oc = out + x_off;
        for (int64_t t = t0 + threadIdx.x; t < t0 + BM_PER_WG && t < n; t += THREADS) {
            float ra, rb;
            rs_output2(RsLinear{ac}, m, RsLinear{bc}, mp, t < vb, seg, scale, w, nwin, num_table, index_step, t, &ra, &rb);
            const float g = sc ? band_gain_at([sc](int64_t j) { return sc[j]; }, band_gain_pos(t, frame), J) : 1.f;
            const float h = xc[t] - ra;
            oc[t] = fmaf(g, h, rb);
        }
    }
}

template <int THREADS>
static int bm_launch(unsigned grid, size_t lds, hipStream_t st, const float* x, const float* a, const float* b, const float* gains,
                     const int64_t* tab, int nclips, int64_t total_x, int64_t total_a, int64_t total_b, int64_t total_g,
                     int64_t total_tiles, int64_t max_n, const RsSegs& seg, double ratio, double scale, const float* win, int nwin,
                     int num_table, int index_step, int hop, float* out) {
    static sos_device_once attr_once;
    if (sos_per_device_once(attr_once, [] {
            if (hipFuncSetAttribute((const void*)resample_merge_kernel<THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024) != hipSuccess) {
                sos_set_error("sos_resample_merge_batch_f32: cannot raise the dynamic LDS limit");
                return (int)SOS_ELAUNCH;
            }
            return (int)SOS_OK;
        }))
        return SOS_ELAUNCH;
    hipLaunchKernelGGL(resample_merge_kernel<THREADS>, dim3(grid), dim3(THREADS), lds, st, x, a, b, gains, tab, nclips, total_x,
                       total_a, total_b, total_g, total_tiles, max_n, seg, ratio, scale, win, nwin, num_table, index_step, hop, out);
    return sos_check_launch("sos_resample_merge_batch_f32");
}

extern "C" int sos_resample_merge_batch_f32(const float* x, const float* a, const float* b, const float* gains, const int64_t* table,
                                            const int64_t* table_host, int nclips, double ratio, const float* win, int nwin,
                                            int num_table, int hop, float* out, sos_stream_t stream) {
    if (!x || !a || !b || !table || !table_host || !win || !out) {
        sos_set_error("sos_resample_merge_batch_f32: null pointer");
        return SOS_EINVAL;
    }
    if (nclips < 1 || nclips > RAGGED_MAX_CLIPS || !(ratio > 0.0) || nwin < 2 || num_table < 1 || hop < 1 ||
        (size_t)(nwin + 1) * sizeof(float) > 160 * 1024) {
        sos_set_error("sos_resample_merge_batch_f32: bad args (1 .. 65535 clips, got %d; ratio=%g, hop=%d: at least 1; nwin=%d: "
                      "(nwin + 1) * 4 bytes must fit the 160 KB LDS)", nclips, ratio, hop, nwin);
        return SOS_EINVAL;
    }
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const int index_step = (int)(scale * (double)num_table);
    if (index_step < 1) {
        sos_set_error("sos_resample_merge_batch_f32: ratio %g too small for a %d-point table", ratio, num_table);
        return SOS_EINVAL;
    }
    const int64_t *x_off = table_host, *n = x_off + nclips, *a_off = n + nclips, *m = a_off + nclips, *b_off = m + nclips,
                  *mp = b_off + nclips, *g_off = mp + nclips, *J = g_off + nclips, *tile0 = J + nclips;
    int64_t total_x = 0, total_a = 0, total_b = 0, total_g = 0, total_tiles = 0, max_n = 0;
    for (int c = 0; c < nclips; ++c) {
        if (n[c] < 1 || n[c] > (int64_t)1 << 52 || m[c] < 1 || m[c] > (int64_t)1 << 52 || mp[c] < 1 || mp[c] > m[c]) {
            sos_set_error("sos_resample_merge_batch_f32: clip %d has n=%lld, m=%lld, m'=%lld (each at least 1, m' at most m)", c,
                          (long long)n[c], (long long)m[c], (long long)mp[c]);
            return SOS_EINVAL;
        }
        const int64_t covered = (int64_t)((double)m[c] * ratio);      // resampy's output length for a, as sos_resample_f32 computes it
        if (covered < n[c]) {
            sos_set_error("sos_resample_merge_batch_f32: clip %d has n=%lld frames but its m=%lld low-rate samples cover %lld at "
                          "ratio %g", c, (long long)n[c], (long long)m[c], (long long)covered, ratio);
            return SOS_EINVAL;
        }
        if (gains && J[c] != (m[c] - 1) / hop + 1) {
            sos_set_error("sos_resample_merge_batch_f32: clip %d has %lld gains (m=%lld, hop=%d: %lld expected)", c, (long long)J[c],
                          (long long)m[c], hop, (long long)((m[c] - 1) / hop + 1));
            return SOS_EINVAL;
        }
        if (x_off[c] < total_x || a_off[c] < total_a || b_off[c] < total_b || (gains && g_off[c] < total_g) ||
            tile0[c] != total_tiles || x_off[c] > INT64_MAX / 8 || a_off[c] > INT64_MAX / 8 || b_off[c] > INT64_MAX / 8 ||
            (gains && g_off[c] > INT64_MAX / 8)) {
            sos_set_error("sos_resample_merge_batch_f32: clip %d overlaps its predecessor or is out of order (x %lld, a %lld, b %lld, "
                          "gains %lld, first tile %lld where %lld is expected)", c, (long long)x_off[c], (long long)a_off[c],
                          (long long)b_off[c], (long long)g_off[c], (long long)tile0[c], (long long)total_tiles);
            return SOS_EINVAL;
        }
        total_x = x_off[c] + n[c];
        total_a = a_off[c] + m[c];
        total_b = b_off[c] + mp[c];
        if (gains) total_g = g_off[c] + J[c];
        total_tiles += (n[c] + BM_PER_WG - 1) / BM_PER_WG;
        max_n = std::max(max_n, n[c]);
    }
    RsSegs seg;
    if (rs_build_segments(1.0 / ratio, max_n, &seg) != 0) {
        sos_set_error("sos_resample_merge_batch_f32: time register needs more than %d segments", RS_MAXSEG);
        return SOS_ENOSPC;
    }
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 1) {
        sos_set_error("sos_resample_merge_batch_f32: cannot read the number of compute units");
        return SOS_ELAUNCH;
    }
    const unsigned grid = (unsigned)(total_tiles < cus ? total_tiles : cus);
    const size_t lds = (size_t)(nwin + 1) * sizeof(float);
    return bm_launch<BM_THREADS>(grid, lds, (hipStream_t)stream, x, a, b, gains, table, nclips, total_x, total_a, total_b, total_g,
                                 total_tiles, max_n, seg, ratio, scale, win, nwin, num_table, index_step, hop, out);
}
