// wave_io.hip -- the front door of both models: decoded PCM -> mono f32 -> band-limited resampling to the
// model rate.
//
// Reference call sites: `librosa.load(path, sr=14000)` (M1/dataset.py:226, M2/predict.py:288,297,303,
// M2/dataset.py) = soundfile decode (integer PCM / 2^(bits-1)) -> to_mono (mean over channels) ->
// resampy.resample(filter='kaiser_best') -> zero-pad to ceil(n * ratio).  resampy is a third-party dependency
// that is absent here (requirements.txt: librosa==0.7.1 -> resampy>=0.2.2); these kernels follow its published
// algorithm (Smith's band-limited interpolation: a Kaiser-windowed sinc tabulated at 512 points per zero
// crossing, linearly interpolated, left wing + right wing per output sample).
//
// resample_kernel: one output sample per thread; the filter half-window (32 769 + 1 floats = 128 KB) lives
// in LDS, so the ~2 x 202 taps of an output at 44.1 -> 14 kHz cost one ds_read2_b32 (w[o], w[o+1]) and one
// L1-resident input read each.  A workgroup walks RS_PER_WG consecutive outputs to amortise the table load.
#include "resample_launch.h"
#include "pcm_core.h"
#include <stdlib.h>

#define RS_THREADS 256
#define RS_PER_WG 4096          // = SOS_RESAMPLE_CHUNK of include/sos_hip.h
#define RS_BATCH_THREADS 1024   // the batch kernel's workgroup (EXPERIMENTS.md 3.4)

// Pcm<T>::cvt, the sample-to-float rule: pcm_core.h (shared with pcm_io.hip)
// interleaved [n_frames][channels] -> mono f32 (np.mean over channels of the f32 samples)
template <typename T>
__global__ void pcm_to_mono_kernel(const T* __restrict__ pcm, int channels, int64_t n_frames, float* __restrict__ out) {
    const float inv = 1.0f / (float)channels;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_frames; i += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int c = 0; c < channels; ++c) s += Pcm<T>::cvt(pcm[i * channels + c]);
        out[i] = channels == 1 ? s : s * inv;
    }
}

static unsigned pcm_mono_grid(int64_t n_frames) {
    return (unsigned)((n_frames + RS_THREADS - 1) / RS_THREADS < 4096 ? (n_frames + RS_THREADS - 1) / RS_THREADS : 4096);
}

extern "C" int sos_pcm_to_mono_f32(const void* pcm, int format, int channels, int64_t n_frames, float* out,
                                   sos_stream_t stream) {
    if (!pcm || !out || channels < 1 || channels > 64 || n_frames < 1) {
        sos_set_error("sos_pcm_to_mono_f32: bad args (channels=%d, n_frames=%lld)", channels, (long long)n_frames);
        return SOS_EINVAL;
    }
    const unsigned grid = pcm_mono_grid(n_frames);
    hipStream_t st = (hipStream_t)stream;
    switch (format) {
    case SOS_PCM_S16: hipLaunchKernelGGL(pcm_to_mono_kernel<int16_t>, dim3(grid), dim3(RS_THREADS), 0, st, (const int16_t*)pcm, channels, n_frames, out); break;
    case SOS_PCM_S32: hipLaunchKernelGGL(pcm_to_mono_kernel<int32_t>, dim3(grid), dim3(RS_THREADS), 0, st, (const int32_t*)pcm, channels, n_frames, out); break;
    case SOS_PCM_U8: hipLaunchKernelGGL(pcm_to_mono_kernel<uint8_t>, dim3(grid), dim3(RS_THREADS), 0, st, (const uint8_t*)pcm, channels, n_frames, out); break;
    case SOS_PCM_F32: hipLaunchKernelGGL(pcm_to_mono_kernel<float>, dim3(grid), dim3(RS_THREADS), 0, st, (const float*)pcm, channels, n_frames, out); break;
    default: sos_set_error("sos_pcm_to_mono_f32: unknown sample format %d", format); return SOS_EINVAL;
    }
    return sos_check_launch("sos_pcm_to_mono_f32");
}

// the same kernel over G.711 code bytes (pcm_core.h's expansion): the same mean expression
extern "C" int sos_g711_to_mono_f32(const void* codes, int law, int channels, int64_t n_frames, float* out, sos_stream_t stream) {
    if (!codes || !out || channels < 1 || channels > 64 || n_frames < 1) {
        sos_set_error("sos_g711_to_mono_f32: bad args (channels=%d, n_frames=%lld)", channels, (long long)n_frames);
        return SOS_EINVAL;
    }
    const unsigned grid = pcm_mono_grid(n_frames);
    hipStream_t st = (hipStream_t)stream;
    switch (law) {
    case SOS_G711_ALAW: hipLaunchKernelGGL(pcm_to_mono_kernel<G711A>, dim3(grid), dim3(RS_THREADS), 0, st, (const G711A*)codes, channels, n_frames, out); break;
    case SOS_G711_ULAW: hipLaunchKernelGGL(pcm_to_mono_kernel<G711U>, dim3(grid), dim3(RS_THREADS), 0, st, (const G711U*)codes, channels, n_frames, out); break;
    default: sos_set_error("sos_g711_to_mono_f32: unknown law %d", law); return SOS_EINVAL;
    }
    return sos_check_launch("sos_g711_to_mono_f32");
}

// The time register (RsSegs, rs_build_segments) and the arithmetic of one output (rs_output): resample_core.h; what sits around
// the output loop on both sides of the launch: resample_launch.h.
extern "C" int sos_resample_time_segments(double ratio, int64_t n_out, int64_t* k0, double* s0, double* d, int capacity) {
    RsSegs g;
    if (!(ratio > 0.0) || n_out < 1 || !k0 || !s0 || !d) { sos_set_error("sos_resample_time_segments: bad args"); return SOS_EINVAL; }
    if (rs_build_segments(1.0 / ratio, n_out, &g) != 0 || g.n > capacity) {
        sos_set_error("sos_resample_time_segments: more than %d segments", capacity < RS_MAXSEG ? capacity : RS_MAXSEG);
        return SOS_ENOSPC;
    }
    for (int i = 0; i < g.n; ++i) { k0[i] = g.k0[i]; s0[i] = g.s0[i]; d[i] = g.d[i]; }
    return g.n;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, int64_t n_in, RsSegs seg,
                                                              double scale, const float* __restrict__ win, int nwin,
                                                              int num_table, int index_step, float* __restrict__ out,
                                                              int64_t n_out, int64_t n_valid) {
    extern __shared__ float w[];
    rs_load_window<RS_THREADS>(w, win, nwin);
    const int64_t t0 = (int64_t)blockIdx.x * RS_PER_WG;
    for (int64_t t = t0 + threadIdx.x; t < t0 + RS_PER_WG && t < n_out; t += RS_THREADS)      // t >= n_valid: librosa
        out[t] = t < n_valid ? rs_output(RsLinear{x}, n_in, seg, scale, w, nwin, num_table, index_step, t) : 0.f;   // fix_length's zeros
}

// The same for a ragged batch.  Table int64 [6][nclips]: clip c is x[tab[0][c] .. + tab[1][c]) -> out[tab[2][c] .. + tab[3][c]),
// of which the first tab[4][c] are resampled; tab[5][c] = its first tile in the list of all (clip, RS_PER_WG outputs) tiles.
struct RsBatchClip { int64_t in_off, n_in, out_off, n_out, n_valid, tile0; };
__host__ __device__ static inline RsBatchClip rs_batch_row(const int64_t* tab, int64_t nclips, int64_t c) {
    return {tab[c], tab[nclips + c], tab[2 * nclips + c], tab[3 * nclips + c], tab[4 * nclips + c], tab[5 * nclips + c]};
}
// Why `tile` of a clip cannot be followed (0: it can): the rule of ragged.h against the totals the host summed from its own
// table (total_in / total_out samples, the largest n_valid), for the kernel's skip and the host's refusal alike.
enum { RSB_OK = 0, RSB_INPUT, RSB_OUTPUT, RSB_VALID, RSB_TILE };
__host__ __device__ static inline int rs_batch_why(const RsBatchClip& e, int64_t total_in, int64_t total_out, int64_t max_valid,
                                                   int64_t tile) {
    if (!ragged_clip_inside(e.in_off, e.n_in, total_in) || e.n_in < 1) return RSB_INPUT;
    if (!ragged_clip_inside(e.out_off, e.n_out, total_out) || e.n_out < 1) return RSB_OUTPUT;
    if (e.n_valid < 0 || e.n_valid > e.n_out || e.n_valid > max_valid) return RSB_VALID;
    const int64_t t0 = (tile - e.tile0) * RS_PER_WG;
    return t0 < 0 || t0 >= e.n_out ? RSB_TILE : RSB_OK;
}

// At most one workgroup per CU fits beside the window, so the grid is one workgroup per CU that loads the window ONCE and
// walks the tiles gridDim.x apart: a mix of short and long clips keeps every CU busy, and the 128 KB load is paid per CU, not
// per tile.  Every bound is the clip's own (rs_output sees the clip as its whole signal); the time register starts at 0 for
// each clip, so `seg`, built for the largest n_valid, serves all.  The table is device data: a tile that rs_batch_why refuses
// is skipped, never followed.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void resample_batch_kernel(const float* __restrict__ x, const int64_t* __restrict__ tab,
                                                                 int nclips, int64_t total_in, int64_t total_out,
                                                                 int64_t total_tiles, int64_t max_valid, RsSegs seg,
                                                                 double scale, const float* __restrict__ win, int nwin,
                                                                 int num_table, int index_step, float* __restrict__ out) {
    extern __shared__ float w[];
    rs_load_window<THREADS>(w, win, nwin);
    for (int64_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const RsBatchClip e = rs_batch_row(tab, nclips, rs_clip_of_tile(tab + 5 * (int64_t)nclips, nclips, tile));
        if (rs_batch_why(e, total_in, total_out, max_valid, tile) != RSB_OK) continue;
        const int64_t t0 = (tile - e.tile0) * RS_PER_WG;
        const float* xc = x + e.in_off;
        float* oc = out + e.out_off;
        for (int64_t t = t0 + threadIdx.x; t < t0 + RS_PER_WG && t < e.n_out; t += THREADS)
            oc[t] = t < e.n_valid ? rs_output(RsLinear{xc}, e.n_in, seg, scale, w, nwin, num_table, index_step, t) : 0.f;
    }
}

extern "C" int sos_resample_f32(const float* x, int64_t n_in, double ratio, const float* win, int nwin, int num_table,
                                float* out, int64_t n_out, sos_stream_t stream) {
    const char* who = "sos_resample_f32";
    if (!x || !win || !out || n_in < 1 || n_out < 1) {
        sos_set_error("%s: bad args (n_in=%lld, n_out=%lld)", who, (long long)n_in, (long long)n_out);
        return SOS_EINVAL;
    }
    RsFilter f;
    if (!rs_filter(who, ratio, nwin, num_table, true, &f)) return SOS_EINVAL;
    int64_t n_valid = (int64_t)((double)n_in * ratio);      // resampy's output length; the rest is librosa's padding
    if (n_valid > n_out) n_valid = n_out;
    RsSegs seg;
    if (const int rc = rs_segments(who, ratio, n_valid > 0 ? n_valid : 1, &seg)) return rc;
    const unsigned grid = (unsigned)((n_out + RS_PER_WG - 1) / RS_PER_WG);      // a workgroup per tile, each loads the window
    return rs_launch<resample_kernel>(who, grid, RS_THREADS, f.lds, stream, x, n_in, seg, f.scale, win, nwin, num_table, f.index_step,
                                      out, n_out, n_valid);
}

extern "C" int sos_resample_batch_f32(const float* x, const int64_t* table, const int64_t* table_host, int nclips, double ratio,
                                      const float* win, int nwin, int num_table, float* out, sos_stream_t stream) {
    const char* who = "sos_resample_batch_f32";
    if (!x || !table || !table_host || !win || !out) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (nclips < 1 || nclips > RAGGED_MAX_CLIPS) { sos_set_error("%s: bad args (1 .. 65535 clips, got %d)", who, nclips); return SOS_EINVAL; }
    RsFilter f;
    if (!rs_filter(who, ratio, nwin, num_table, true, &f)) return SOS_EINVAL;
    int64_t total_in = 0, total_out = 0, total_tiles = 0, max_valid = 0;
    for (int c = 0; c < nclips; ++c) {
        const RsBatchClip e = rs_batch_row(table_host, nclips, c);
        if (e.n_in < 1 || e.n_in > (int64_t)1 << 52) {
            sos_set_error("%s: clip %d has n_in=%lld", who, c, (long long)e.n_in);
            return SOS_EINVAL;
        }
        int64_t want = (int64_t)((double)e.n_in * ratio);        // resampy's output length, as sos_resample_f32 computes it
        if (want > e.n_out) want = e.n_out;
        if (e.n_valid < 1 || e.n_valid != want) {
            sos_set_error("%s: clip %d has n_valid=%lld (n_in=%lld, n_out=%lld, ratio=%g: %lld expected; at least 1)", who, c,
                          (long long)e.n_valid, (long long)e.n_in, (long long)e.n_out, ratio, (long long)want);
            return SOS_EINVAL;
        }
        if (e.in_off < total_in || e.out_off < total_out || e.tile0 != total_tiles || e.in_off > INT64_MAX / 8 ||
            e.out_off > INT64_MAX / 8 || e.n_out > (int64_t)1 << 52) {
            sos_set_error("%s: clip %d overlaps its predecessor or is out of order (in %lld, out %lld, first tile %lld where %lld is "
                          "expected)", who, c, (long long)e.in_off, (long long)e.out_off, (long long)e.tile0, (long long)total_tiles);
            return SOS_EINVAL;
        }
        total_in = e.in_off + e.n_in;
        total_out = e.out_off + e.n_out;
        total_tiles += (e.n_out + RS_PER_WG - 1) / RS_PER_WG;
        if (e.n_valid > max_valid) max_valid = e.n_valid;
    }
    for (int c = 0; c < nclips; ++c) {                           // what the kernel will ask of each clip, first tile and last
        const RsBatchClip e = rs_batch_row(table_host, nclips, c);
        for (const int64_t tile : {e.tile0, e.tile0 + (e.n_out - 1) / RS_PER_WG})
            if (const int why = rs_batch_why(e, total_in, total_out, max_valid, tile)) {
                sos_set_error("%s: clip %d lies outside the totals of the table (rule %d, tile %lld)", who, c, why, (long long)tile);
                return SOS_EINVAL;
            }
    }
    RsSegs seg;
    if (const int rc = rs_segments(who, ratio, max_valid, &seg)) return rc;
    const unsigned grid = rs_grid(who, total_tiles);
    if (!grid) return SOS_ELAUNCH;
    // workgroup size: A/B switch (read per call: tools/wave_io_batch_bench.py flips it; EXPERIMENTS.md 3.4).  The results do
    // not depend on it.
    const char* env_threads = getenv("SOS_RESAMPLE_BATCH_THREADS");
    const int threads = env_threads ? atoi(env_threads) : RS_BATCH_THREADS;
#define RS_GO(T) rs_launch<resample_batch_kernel<T>>(who, grid, T, f.lds, stream, x, table, nclips, total_in, total_out, total_tiles, \
                                                     max_valid, seg, f.scale, win, nwin, num_table, f.index_step, out)
    return threads == 256 ? RS_GO(256) : threads == 512 ? RS_GO(512) : RS_GO(1024);
#undef RS_GO
}
