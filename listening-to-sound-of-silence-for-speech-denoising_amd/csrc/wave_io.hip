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
#include "resample_core.h"
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

// The time register (RsSegs, rs_build_segments) and the arithmetic of one output (rs_output): resample_core.h.
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
    for (int i = threadIdx.x; i <= nwin; i += RS_THREADS) w[i] = win[i < nwin ? i : nwin - 1];
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * RS_PER_WG;
    for (int64_t t = t0 + threadIdx.x; t < t0 + RS_PER_WG && t < n_out; t += RS_THREADS)      // t >= n_valid: librosa
        out[t] = t < n_valid ? rs_output(RsLinear{x}, n_in, seg, scale, w, nwin, num_table, index_step, t) : 0.f;   // fix_length's zeros
}

// The same for a ragged batch: clip c is x[tab[0][c] .. + tab[1][c]) -> out[tab[2][c] .. + tab[3][c]), of which the first
// tab[4][c] are resampled; tab[5][c] = its first tile in the list of all (clip, RS_PER_WG outputs) tiles.  At most one
// workgroup per CU fits beside the window, so the grid is one workgroup per CU that loads the window ONCE and walks the
// tiles gridDim.x apart: a mix of short and long clips keeps every CU busy, and the 128 KB load is paid per CU, not per
// tile.  Every bound is the clip's own (rs_output sees the clip as its whole signal); the time register starts at 0 for
// each clip, so `seg`, built for the largest n_valid, serves all.  The table is device data: an entry that does not
// lie inside the totals the host validated (total_in / total_out samples, max_valid) is skipped, never followed.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void resample_batch_kernel(const float* __restrict__ x, const int64_t* __restrict__ tab,
                                                                 int nclips, int64_t total_in, int64_t total_out,
                                                                 int64_t total_tiles, int64_t max_valid, RsSegs seg,
                                                                 double scale, const float* __restrict__ win, int nwin,
                                                                 int num_table, int index_step, float* __restrict__ out) {
    extern __shared__ float w[];
    for (int i = threadIdx.x; i <= nwin; i += THREADS) w[i] = win[i < nwin ? i : nwin - 1];
    __syncthreads();
    const int64_t* tile0 = tab + 5 * (int64_t)nclips;
    for (int64_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        int lo = 0, hi = nclips - 1;                          // the last clip whose first tile is <= tile
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tile0[mid] <= tile) lo = mid; else hi = mid - 1;
        }
        const int64_t in_off = tab[lo], n_in = tab[nclips + lo], out_off = tab[2 * (int64_t)nclips + lo];
        const int64_t n_out = tab[3 * (int64_t)nclips + lo], n_valid = tab[4 * (int64_t)nclips + lo];
        const int64_t t0 = (tile - tile0[lo]) * RS_PER_WG;
        if (!ragged_clip_inside(in_off, n_in, total_in) || n_in < 1 || !ragged_clip_inside(out_off, n_out, total_out) ||
            n_out < 1 || n_valid < 0 || n_valid > n_out || n_valid > max_valid || t0 < 0 || t0 >= n_out)
            continue;
        const float* xc = x + in_off;
        float* oc = out + out_off;
        for (int64_t t = t0 + threadIdx.x; t < t0 + RS_PER_WG && t < n_out; t += THREADS)
            oc[t] = t < n_valid ? rs_output(RsLinear{xc}, n_in, seg, scale, w, nwin, num_table, index_step, t) : 0.f;
    }
}

extern "C" int sos_resample_f32(const float* x, int64_t n_in, double ratio, const float* win, int nwin, int num_table,
                                float* out, int64_t n_out, sos_stream_t stream) {
    if (!x || !win || !out || n_in < 1 || n_out < 1 || !(ratio > 0.0) || nwin < 2 || num_table < 1 ||
        (size_t)(nwin + 1) * sizeof(float) > 160 * 1024) {
        sos_set_error("sos_resample_f32: bad args (n_in=%lld, n_out=%lld, ratio=%g, nwin=%d)", (long long)n_in,
                      (long long)n_out, ratio, nwin);
        return SOS_EINVAL;
    }
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const int index_step = (int)(scale * (double)num_table);
    if (index_step < 1) { sos_set_error("sos_resample_f32: ratio %g too small for a %d-point table", ratio, num_table); return SOS_EINVAL; }
    int64_t n_valid = (int64_t)((double)n_in * ratio);      // resampy's output length; the rest is librosa's padding
    if (n_valid > n_out) n_valid = n_out;
    const size_t lds = (size_t)(nwin + 1) * sizeof(float);
    static sos_device_once attr_once;
    if (sos_per_device_once(attr_once, [] {
            if (hipFuncSetAttribute((const void*)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
                sos_set_error("sos_resample_f32: cannot raise the dynamic LDS limit");
                return (int)SOS_ELAUNCH;
            }
            return (int)SOS_OK;
        }))
        return SOS_ELAUNCH;
    RsSegs seg;
    if (rs_build_segments(1.0 / ratio, n_valid > 0 ? n_valid : 1, &seg) != 0) {
        sos_set_error("sos_resample_f32: time register needs more than %d segments", RS_MAXSEG);
        return SOS_ENOSPC;
    }
    const unsigned grid = (unsigned)((n_out + RS_PER_WG - 1) / RS_PER_WG);
    hipLaunchKernelGGL(resample_kernel, dim3(grid), dim3(RS_THREADS), lds, (hipStream_t)stream, x, n_in, seg, scale,
                       win, nwin, num_table, index_step, out, n_out, n_valid);
    return sos_check_launch("sos_resample_f32");
}

template <int THREADS>
static int rs_launch_batch(unsigned grid, size_t lds, hipStream_t st, const float* x, const int64_t* tab, int nclips,
                           int64_t total_in, int64_t total_out, int64_t total_tiles, int64_t max_valid, const RsSegs& seg,
                           double scale, const float* win, int nwin, int num_table, int index_step, float* out) {
    static sos_device_once attr_once;
    if (sos_per_device_once(attr_once, [] {
            if (hipFuncSetAttribute((const void*)resample_batch_kernel<THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024) != hipSuccess) {
                sos_set_error("sos_resample_batch_f32: cannot raise the dynamic LDS limit");
                return (int)SOS_ELAUNCH;
            }
            return (int)SOS_OK;
        }))
        return SOS_ELAUNCH;
    hipLaunchKernelGGL(resample_batch_kernel<THREADS>, dim3(grid), dim3(THREADS), lds, st, x, tab, nclips, total_in, total_out,
                       total_tiles, max_valid, seg, scale, win, nwin, num_table, index_step, out);
    return sos_check_launch("sos_resample_batch_f32");
}

extern "C" int sos_resample_batch_f32(const float* x, const int64_t* table, const int64_t* table_host, int nclips, double ratio,
                                      const float* win, int nwin, int num_table, float* out, sos_stream_t stream) {
    if (!x || !table || !table_host || !win || !out) { sos_set_error("sos_resample_batch_f32: null pointer"); return SOS_EINVAL; }
    if (nclips < 1 || nclips > RAGGED_MAX_CLIPS || !(ratio > 0.0) || nwin < 2 || num_table < 1 ||
        (size_t)(nwin + 1) * sizeof(float) > 160 * 1024) {
        sos_set_error("sos_resample_batch_f32: bad args (1 .. 65535 clips, got %d; ratio=%g, nwin=%d: (nwin + 1) * 4 bytes must "
                      "fit the 160 KB LDS)", nclips, ratio, nwin);
        return SOS_EINVAL;
    }
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const int index_step = (int)(scale * (double)num_table);
    if (index_step < 1) {
        sos_set_error("sos_resample_batch_f32: ratio %g too small for a %d-point table", ratio, num_table);
        return SOS_EINVAL;
    }
    const int64_t *in_off = table_host, *n_in = in_off + nclips, *out_off = n_in + nclips, *n_out = out_off + nclips,
                  *n_valid = n_out + nclips, *tile0 = n_valid + nclips;
    int64_t total_in = 0, total_out = 0, total_tiles = 0, max_valid = 0;
    for (int c = 0; c < nclips; ++c) {
        if (n_in[c] < 1 || n_in[c] > (int64_t)1 << 52) {
            sos_set_error("sos_resample_batch_f32: clip %d has n_in=%lld", c, (long long)n_in[c]);
            return SOS_EINVAL;
        }
        int64_t want = (int64_t)((double)n_in[c] * ratio);       // resampy's output length, as sos_resample_f32 computes it
        if (want > n_out[c]) want = n_out[c];
        if (n_valid[c] < 1 || n_valid[c] != want) {
            sos_set_error("sos_resample_batch_f32: clip %d has n_valid=%lld (n_in=%lld, n_out=%lld, ratio=%g: %lld expected; "
                          "at least 1)", c, (long long)n_valid[c], (long long)n_in[c], (long long)n_out[c], ratio, (long long)want);
            return SOS_EINVAL;
        }
        if (in_off[c] < total_in || out_off[c] < total_out || tile0[c] != total_tiles ||
            in_off[c] > INT64_MAX / 8 || out_off[c] > INT64_MAX / 8 || n_out[c] > (int64_t)1 << 52) {
            sos_set_error("sos_resample_batch_f32: clip %d overlaps its predecessor or is out of order (in %lld, out %lld, first "
                          "tile %lld where %lld is expected)", c, (long long)in_off[c], (long long)out_off[c],
                          (long long)tile0[c], (long long)total_tiles);
            return SOS_EINVAL;
        }
        total_in = in_off[c] + n_in[c];
        total_out = out_off[c] + n_out[c];
        total_tiles += (n_out[c] + RS_PER_WG - 1) / RS_PER_WG;
        if (n_valid[c] > max_valid) max_valid = n_valid[c];
    }
    RsSegs seg;
    if (rs_build_segments(1.0 / ratio, max_valid, &seg) != 0) {
        sos_set_error("sos_resample_batch_f32: time register needs more than %d segments", RS_MAXSEG);
        return SOS_ENOSPC;
    }
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 1) {
        sos_set_error("sos_resample_batch_f32: cannot read the number of compute units");
        return SOS_ELAUNCH;
    }
    const unsigned grid = (unsigned)(total_tiles < cus ? total_tiles : cus);
    const size_t lds = (size_t)(nwin + 1) * sizeof(float);
    // workgroup size: A/B switch (read per call: tools/wave_io_batch_bench.py flips it; EXPERIMENTS.md 3.4).  The results do
    // not depend on it.
    const char* env_threads = getenv("SOS_RESAMPLE_BATCH_THREADS");
    const int threads = env_threads ? atoi(env_threads) : RS_BATCH_THREADS;
    hipStream_t st = (hipStream_t)stream;
#define RS_GO(T) rs_launch_batch<T>(grid, lds, st, x, table, nclips, total_in, total_out, total_tiles, max_valid, seg, scale, win, \
                                    nwin, num_table, index_step, out)
    return threads == 256 ? RS_GO(256) : threads == 512 ? RS_GO(512) : RS_GO(1024);
#undef RS_GO
}
