// ragged_mix.hip -- noisy speech out of clean speech for a ragged batch of clips: add_signals with one noise (M2/tools.py:217-276)
// composed with what the hand-off does around it (float64 restatement: tests/mix_reference.py).  Per clip of n samples:
//   s[j] = clip[j] (1 - mask_sample(j)) where the clip has frame decisions (mask_rule.h, the rule of sos_bits_to_mask)
//   z[j] = noise[noff + j] for j < nz, 0 for nz <= j < n                   (the zero-filled crop of add_noise_to_audio)
//   Es = sum s^2, Ez = sum z^2 (f64);  gain = 1 if Es == 0 or Ez == 0, else sqrt(Es / 10^(snr / 10)) / sqrt(Ez)
//   m = s + gain z;  peak = max |m|;  inv = norm / peak if norm != 0 and peak != 0, else 1
//   mixed = m inv, clean = s inv, noise_out = gain z inv, back to back at the clip's offset like the input.
// A clip is cut into chunks of MIX_CHUNK samples counted from ITS first sample; thread t of a workgroup takes the samples
// 1024 q + 4 t .. + 3 of a chunk, q = 0 .. 3, in rising order.  Four launches, whatever the number of clips, no host
// synchronisation, no atomics:
//   mix_plan_kernel    one workgroup: the bounds rule on every clip of the DEVICE table (status -1 and no work for one that
//                      fails) and a scan of the chunk counts: where each clip's chunk results lie in the workspace.
//   mix_energy_kernel  grid (chunks, clips): s (the mask rule is evaluated here and nowhere else) into `clean`; the chunk's
//                      sums of s^2 and z^2, f64, a fixed tree.
//   mix_peak_kernel    every workgroup first adds the clip's chunk sums (thread t the chunks t, t + 256, ... in rising order,
//                      then the tree) and takes the gain; the chunk's max |s + gain z| in f64 (inv is then one f32 rounding
//                      away from the float64 restatement's).
//   mix_write_kernel   every workgroup first takes the clip's peak over its chunks and inv; the three outputs.
// gain and inv are applied as f32 factors rounded from f64 (out reports those f32 values); the m that is written is one fmaf.  Which workgroup
// works on which chunk, and whether a clip's address allows 16-byte accesses (ragged_load4 / ragged_store4), changes no
// value: a clip has the same bits alone, in any batch, at any offset and in any order.
// Bounds: the rule of ragged.h -- the host refuses a table entry outside what it summed from the _host copies; the kernels
// follow the DEVICE tables and parameters (mix_clip_ok).  Crops of different clips may overlap in `noise`: each is checked
// against [0, noise_total) on its own.  The input clips must not overlap the three output buffers.
#include "ragged.h"
#include "mask_rule.h"

#define MIX_CHUNK SOS_MIX_CHUNK         // samples per chunk: 4 x (MT threads x 4 samples)
#define MIX_STEPS (MIX_CHUNK / (MT * 4))
#define MIX_MAX_GRID 1024               // workgroups along a clip's chunks (they stride over what the grid does not cover)
#define MIX_MAX_SAMPLES (1LL << 40)     // samples per call: the sum of 65535 chunk counts stays far inside int64
#define MIX_OUT 6                       // f64 per clip: Es, Ez, gain, peak, inv, status
static_assert(MIX_STEPS * MT * 4 == MIX_CHUNK, "a chunk is a whole number of workgroup steps");

__host__ __device__ static inline int64_t mix_chunks(int64_t n) { return (n - 1) / MIX_CHUNK + 1; }       // n >= 1
__host__ __device__ static inline bool mix_finite(double v) { return v - v == 0.0; }
// no frame decisions (0), or more than one sample per frame
__host__ __device__ static inline bool mix_ratio_ok(double ratio) { return ratio == 0.0 || (ratio > 1.0 && mix_finite(ratio)); }
// the crop [noff, noff + nz) lies inside the noise buffer and is no longer than the clip
__host__ __device__ static inline bool mix_crop_ok(int64_t noff, int64_t nz, int64_t n, int64_t noise_total) {
    return nz <= n && ragged_clip_inside(noff, nz, noise_total);
}

// what the plan kernel asks of a clip of the device tables before anything is read or written for it
__device__ static inline bool mix_clip_ok(const RaggedClip& c, const int64_t* nt, const double* p, bool have_bits, int64_t total,
                                          int64_t total_frames, int64_t noise_total) {
    if (c.n < 1 || !ragged_clip_inside(c.off, c.n, total) || !mix_crop_ok(nt[0], nt[1], c.n, noise_total)) return false;
    if (!mix_finite(p[0]) || !mix_ratio_ok(p[1])) return false;
    return p[1] == 0.0 || (have_bits && ragged_clip_inside(c.foff, c.frames, total_frames));
}

__global__ __launch_bounds__(MT) void mix_plan_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ noise_table,
                                                      const double* __restrict__ params, int have_bits, int nclips, int64_t total,
                                                      int64_t total_frames, int64_t noise_total, int64_t total_chunks,
                                                      int64_t* __restrict__ first_chunk, double* __restrict__ out) {
    __shared__ int64_t scan[MT];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int base = 0; base < nclips; base += MT) {
        const int b = base + tid;
        int64_t nch = 0;
        if (b < nclips) {
            const RaggedClip c = ragged_clip(table, b);
            if (mix_clip_ok(c, noise_table + 2 * (int64_t)b, params + 2 * (int64_t)b, have_bits != 0, total, total_frames, noise_total))
                nch = mix_chunks(c.n);                                   // n <= total <= MIX_MAX_SAMPLES
        }
        scan[tid] = nch;
        __syncthreads();
        for (int s = 1; s < MT; s <<= 1) {
            const int64_t u = tid >= s ? scan[tid - s] : 0;
            __syncthreads();
            scan[tid] += u;
            __syncthreads();
        }
        const int64_t first = carry + scan[tid] - nch;
        carry += scan[MT - 1];
        if (b < nclips) {
            const bool ok = nch > 0 && first + nch <= total_chunks;      // the workspace holds total_chunks chunk results
            first_chunk[b] = ok ? first : -1;
            if (!ok) {
                double* o = out + (int64_t)b * MIX_OUT;
                o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0; o[4] = 0.0; o[5] = -1.0;
            }
        }
        __syncthreads();                                                 // scan[MT - 1] read before the next tile's scan
    }
}

// what the three passes know of their clip
struct MixClip {
    int64_t n, nz, nch, first;
    const float* z;                     // the crop
    int64_t off;
    bool z_vec;
};
__device__ static inline MixClip mix_clip(const int64_t* table, const int64_t* noise_table, const int64_t* first_chunk,
                                          const float* noise, int64_t b) {
    MixClip m = {};
    m.first = first_chunk[b];
    if (m.first < 0) return m;
    const RaggedClip c = ragged_clip(table, b);
    m.n = c.n;
    m.off = c.off;
    m.nch = mix_chunks(c.n);
    m.nz = noise_table[2 * b + 1];
    m.z = noise + noise_table[2 * b];
    m.z_vec = ragged_aligned16(m.z);
    return m;
}
// the first of this thread's four samples in step q of chunk ch
__device__ __forceinline__ int64_t mix_j0(int64_t ch, int q) { return ch * MIX_CHUNK + ((int64_t)q * MT + threadIdx.x) * 4; }
// z[j0 .. j0 + 4): the crop, zero from its end on
__device__ __forceinline__ void mix_load_noise(const MixClip& m, int64_t j0, float (&z)[4]) {
    z[0] = 0.f; z[1] = 0.f; z[2] = 0.f; z[3] = 0.f;
    ragged_load4(m.z, j0, m.nz, m.z_vec && j0 + 4 <= m.nz, z);
}

__global__ __launch_bounds__(MT) void mix_energy_kernel(const float* __restrict__ x, const int64_t* __restrict__ table,
                                                        const float* __restrict__ noise, const int64_t* __restrict__ noise_table,
                                                        const uint8_t* __restrict__ bits, const double* __restrict__ params,
                                                        const int64_t* __restrict__ first_chunk, float* __restrict__ clean,
                                                        double* __restrict__ esum) {
    __shared__ double red[MT];
    const int64_t b = blockIdx.y;
    const MixClip m = mix_clip(table, noise_table, first_chunk, noise, b);
    if (m.first < 0) return;
    const RaggedClip c = ragged_clip(table, b);
    const double ratio = params[2 * b + 1];
    const uint8_t* bc = ratio != 0.0 ? bits + c.foff : nullptr;
    const float* xc = x + m.off;
    float* cc = clean + m.off;
    const bool x_vec = ragged_aligned16(xc), c_vec = ragged_aligned16(cc);
    for (int64_t ch = blockIdx.x; ch < m.nch; ch += gridDim.x) {
        double es = 0.0, ez = 0.0;
#pragma unroll
        for (int q = 0; q < MIX_STEPS; ++q) {
            const int64_t j0 = mix_j0(ch, q);
            if (j0 >= m.n) continue;
            const bool full = j0 + 4 <= m.n;
            float s[4] = {0.f, 0.f, 0.f, 0.f}, z[4];
            ragged_load4(xc, j0, m.n, full && x_vec, s);
            if (bc) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j0 + k < m.n) s[k] *= 1.f - mask_sample(bc, c.frames, ratio, m.n, j0 + k);
            }
            ragged_store4(cc, j0, m.n, full && c_vec, s);
            mix_load_noise(m, j0, z);
#pragma unroll
            for (int k = 0; k < 4; ++k) {                                // (the zeros past the clip's end add nothing)
                es = fma((double)s[k], (double)s[k], es);
                ez = fma((double)z[k], (double)z[k], ez);
            }
        }
        const double Es = block_sum(es, red), Ez = block_sum(ez, red);
        if (threadIdx.x == 0) {
            esum[2 * (m.first + ch)] = Es;
            esum[2 * (m.first + ch) + 1] = Ez;
        }
    }
}

__global__ __launch_bounds__(MT) void mix_peak_kernel(const int64_t* __restrict__ table, const float* __restrict__ noise,
                                                      const int64_t* __restrict__ noise_table, const double* __restrict__ params,
                                                      const int64_t* __restrict__ first_chunk, const float* __restrict__ clean,
                                                      const double* __restrict__ esum, double* __restrict__ peaks,
                                                      double* __restrict__ out) {
    __shared__ double red[MT];
    const int64_t b = blockIdx.y;
    const MixClip m = mix_clip(table, noise_table, first_chunk, noise, b);
    if (m.first < 0 || (int64_t)blockIdx.x >= m.nch) return;
    double es = 0.0, ez = 0.0;
    for (int64_t i = threadIdx.x; i < m.nch; i += MT) {
        es += esum[2 * (m.first + i)];
        ez += esum[2 * (m.first + i) + 1];
    }
    const double Es = block_sum(es, red), Ez = block_sum(ez, red);
    const double gain = (Es == 0.0 || Ez == 0.0) ? 1.0 : sqrt(Es / pow(10.0, params[2 * b] / 10.0)) / sqrt(Ez);
    const float g = (float)gain;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double* o = out + b * MIX_OUT;
        o[0] = Es; o[1] = Ez; o[2] = (double)g;
    }
    const float* sc = clean + m.off;
    const bool s_vec = ragged_aligned16(sc);
    for (int64_t ch = blockIdx.x; ch < m.nch; ch += gridDim.x) {
        double pk = 0.0;
#pragma unroll
        for (int q = 0; q < MIX_STEPS; ++q) {
            const int64_t j0 = mix_j0(ch, q);
            if (j0 >= m.n) continue;
            float s[4] = {0.f, 0.f, 0.f, 0.f}, z[4];
            ragged_load4(sc, j0, m.n, s_vec && j0 + 4 <= m.n, s);
            mix_load_noise(m, j0, z);
#pragma unroll
            for (int k = 0; k < 4; ++k) pk = fmax(pk, fabs(fma(gain, (double)z[k], (double)s[k])));
        }
        const double P = block_max(pk, red);
        if (threadIdx.x == 0) peaks[m.first + ch] = P;
    }
}

__global__ __launch_bounds__(MT) void mix_write_kernel(const int64_t* __restrict__ table, const float* __restrict__ noise,
                                                       const int64_t* __restrict__ noise_table, double norm,
                                                       const int64_t* __restrict__ first_chunk, const double* __restrict__ peaks,
                                                       float* __restrict__ mixed, float* __restrict__ clean,
                                                       float* __restrict__ noise_out, double* __restrict__ out) {
    __shared__ double red[MT];
    const int64_t b = blockIdx.y;
    const MixClip m = mix_clip(table, noise_table, first_chunk, noise, b);
    if (m.first < 0 || (int64_t)blockIdx.x >= m.nch) return;
    double pk = 0.0;
    for (int64_t i = threadIdx.x; i < m.nch; i += MT) pk = fmax(pk, peaks[m.first + i]);
    const double peak = block_max(pk, red);
    double* o = out + b * MIX_OUT;
    const float g = (float)o[2];                                         // mix_peak_kernel's
    const float inv = (norm != 0.0 && peak != 0.0) ? (float)(norm / peak) : 1.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) { o[3] = peak; o[4] = (double)inv; o[5] = 0.0; }
    float* mc = mixed + m.off;
    float* sc = clean + m.off;
    float* nc = noise_out + m.off;
    const bool m_vec = ragged_aligned16(mc), s_vec = ragged_aligned16(sc), n_vec = ragged_aligned16(nc);
    for (int64_t ch = blockIdx.x; ch < m.nch; ch += gridDim.x) {
#pragma unroll
        for (int q = 0; q < MIX_STEPS; ++q) {
            const int64_t j0 = mix_j0(ch, q);
            if (j0 >= m.n) continue;
            const bool full = j0 + 4 <= m.n;
            float s[4] = {0.f, 0.f, 0.f, 0.f}, z[4], mx[4];
            ragged_load4(sc, j0, m.n, full && s_vec, s);
            mix_load_noise(m, j0, z);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mx[k] = fmaf(g, z[k], s[k]) * inv;
                s[k] *= inv;
                z[k] = (g * z[k]) * inv;
            }
            ragged_store4(mc, j0, m.n, full && m_vec, mx);
            ragged_store4(sc, j0, m.n, full && s_vec, s);
            ragged_store4(nc, j0, m.n, full && n_vec, z);
        }
    }
}

// the workspace: int64 first chunk per clip, then f64 {Es, Ez} per chunk, then f64 peak per chunk
struct MixLayout { size_t first, esum, peaks, bytes; };
static MixLayout mix_layout(int64_t chunks, int nclips) {
    RaggedBump ws;
    MixLayout l;
    l.first = ws.take((size_t)nclips * 8);
    l.esum = ws.take((size_t)chunks * 16);
    l.peaks = ws.take((size_t)chunks * 8);
    l.bytes = ws.o;
    return l;
}
// the chunks of the clips of a host table; a clip the launch would refuse by name counts as 0
static int64_t mix_total_chunks(const int64_t* table_host, int nclips, int64_t* longest) {
    int64_t chunks = 0, most = 0;
    for (int b = 0; b < nclips; ++b) {
        const int64_t n = table_host[(int64_t)b * RAGGED_CLIP_COLS + 1];
        if (n < 1 || n > MIX_MAX_SAMPLES) continue;
        chunks += mix_chunks(n);
        most = std::max(most, mix_chunks(n));
    }
    if (longest) *longest = most;
    return chunks;
}

extern "C" int64_t sos_ragged_mix_workspace_bytes(const int64_t* table_host, int nclips) {
    if (!ragged_clips_ok(table_host, nclips)) {
        sos_set_error("sos_ragged_mix_workspace_bytes: bad args (1 .. 65535 clips, got %d)", nclips);
        return -1;
    }
    return (int64_t)mix_layout(mix_total_chunks(table_host, nclips, nullptr), nclips).bytes;
}

extern "C" int sos_ragged_mix_f32(const float* clips, const int64_t* table, const int64_t* table_host, int nclips,
                                  const float* noise, int64_t noise_total, const int64_t* noise_table,
                                  const int64_t* noise_table_host, const uint8_t* bits, const double* params,
                                  const double* params_host, double norm, void* workspace, int64_t workspace_bytes, float* mixed,
                                  float* clean, float* noise_out, double* out, sos_stream_t stream) {
    if (!clips || !table || !table_host || !noise || !noise_table || !noise_table_host || !params || !params_host || !workspace ||
        !mixed || !clean || !noise_out || !out) {
        sos_set_error("sos_ragged_mix_f32: null pointer");
        return SOS_EINVAL;
    }
    if (!ragged_clips_ok(table_host, nclips) || noise_total < 0 || !mix_finite(norm)) {
        sos_set_error("sos_ragged_mix_f32: bad args (1 .. 65535 clips, got %d; %lld noise samples; norm %g)", nclips,
                      (long long)noise_total, norm);
        return SOS_EINVAL;
    }
    RaggedSum ns, nf;
    int bad = std::min(ragged_sum_column(table_host, nclips, RAGGED_CLIP_COLS, 1, 1, MIX_MAX_SAMPLES, &ns),
                       ragged_sum_column(table_host, nclips, RAGGED_CLIP_COLS, 3, 0, INT64_MAX, &nf));
    if (bad < nclips || ns.total > MIX_MAX_SAMPLES) {
        if (bad < nclips) {
            const RaggedClip c = ragged_clip(table_host, bad);
            sos_set_error("sos_ragged_mix_f32: clip %d has %lld samples (at least 1) and %lld frames", bad, (long long)c.n,
                          (long long)c.frames);
        } else {
            sos_set_error("sos_ragged_mix_f32: %lld samples in one call (at most 2^40)", (long long)ns.total);
        }
        return SOS_EINVAL;
    }
    for (int b = 0; b < nclips; ++b) {
        const RaggedClip c = ragged_clip(table_host, b);
        const int64_t noff = noise_table_host[2 * b], nz = noise_table_host[2 * b + 1];
        const double snr = params_host[2 * b], ratio = params_host[2 * b + 1];
        if (!ragged_clip_inside(c.off, c.n, ns.total)) {
            sos_set_error("sos_ragged_mix_f32: clip %d (samples %lld + %lld) lies outside the %lld samples of the table", b,
                          (long long)c.off, (long long)c.n, (long long)ns.total);
            return SOS_EINVAL;
        }
        if (!mix_finite(snr)) {
            sos_set_error("sos_ragged_mix_f32: clip %d has snr %g dB (must be finite)", b, snr);
            return SOS_EINVAL;
        }
        if (!mix_ratio_ok(ratio)) {
            sos_set_error("sos_ragged_mix_f32: clip %d has ratio %g (samples per frame must exceed 1; 0 = no frame decisions)", b,
                          ratio);
            return SOS_EINVAL;
        }
        if (ratio != 0.0 && !bits) {
            sos_set_error("sos_ragged_mix_f32: clip %d has ratio %g but bits is null", b, ratio);
            return SOS_EINVAL;
        }
        if (ratio != 0.0 && !ragged_clip_inside(c.foff, c.frames, nf.total)) {
            sos_set_error("sos_ragged_mix_f32: clip %d (frames %lld + %lld) lies outside the %lld frames of the table", b,
                          (long long)c.foff, (long long)c.frames, (long long)nf.total);
            return SOS_EINVAL;
        }
        if (!mix_crop_ok(noff, nz, c.n, noise_total)) {
            sos_set_error("sos_ragged_mix_f32: clip %d: the noise crop %lld + %lld must lie inside the %lld noise samples and be no "
                          "longer than the clip's %lld samples", b, (long long)noff, (long long)nz, (long long)noise_total,
                          (long long)c.n);
            return SOS_EINVAL;
        }
    }
    int64_t longest = 0;
    const int64_t chunks = mix_total_chunks(table_host, nclips, &longest);
    const MixLayout l = mix_layout(chunks, nclips);
    if (workspace_bytes < (int64_t)l.bytes) {
        sos_set_error("sos_ragged_mix_f32: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)l.bytes);
        return SOS_ENOSPC;
    }
    char* ws = (char*)workspace;
    int64_t* first = (int64_t*)(ws + l.first);
    double* esum = (double*)(ws + l.esum);
    double* peaks = (double*)(ws + l.peaks);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ragged_grid(longest, 1, MIX_MAX_GRID), (unsigned)nclips);
    int rc;
    hipLaunchKernelGGL(mix_plan_kernel, dim3(1), dim3(MT), 0, s, table, noise_table, params, bits ? 1 : 0, nclips, ns.total, nf.total,
                       noise_total, chunks, first, out);
    if ((rc = sos_check_launch("sos_ragged_mix_f32: plan")) != SOS_OK) return rc;
    hipLaunchKernelGGL(mix_energy_kernel, grid, dim3(MT), 0, s, clips, table, noise, noise_table, bits, params, (const int64_t*)first,
                       clean, esum);
    if ((rc = sos_check_launch("sos_ragged_mix_f32: energies")) != SOS_OK) return rc;
    hipLaunchKernelGGL(mix_peak_kernel, grid, dim3(MT), 0, s, table, noise, noise_table, params, (const int64_t*)first,
                       (const float*)clean, (const double*)esum, peaks, out);
    if ((rc = sos_check_launch("sos_ragged_mix_f32: peaks")) != SOS_OK) return rc;
    hipLaunchKernelGGL(mix_write_kernel, grid, dim3(MT), 0, s, table, noise, noise_table, norm, (const int64_t*)first,
                       (const double*)peaks, mixed, clean, noise_out, out);
    return sos_check_launch("sos_ragged_mix_f32: outputs");
}
