// metrics_batch.hip -- the objective measures of M2/metrics.py (everything sos_amd.metrics.evaluate_metrics reports but
// PESQ / STOI) of a ragged batch of (clean, noisy) clip pairs.  One batch is a fixed launch sequence on one stream, no
// allocation, no host synchronisation:
//   mb_plan_kernel         per-clip extents (one thread, a running sum over the clips); frame counts as the reference does
//   mb_totals_kernel       per 4096-sample chunk: f64 partials of sum c^2, sum (c-n)^2, max |c|, sum |n-c|
//   mb_totals_sum_kernel   per clip: one fixed-order reduction over its chunks -> head[b][0..3]
//   mb_keep_count_kernel   per chunk: samples kept by the silence rule, threshold (float)max * 0.03f read from head[b][2]
//   mb_keep_scan_kernel    per clip: exclusive scan over its chunks; kept samples k and the kept-frame count of k
//   mb_keep_scatter_kernel per chunk: order-preserving copy of the kept samples of both signals
//   mb_frames_kernel       per frame of the full signals: frame energies (once, for the three segmental SNRs) and LLR
//   mb_wss_kernel          per frame of the full signals: WSS, the DFT twiddles built once per workgroup
//                          (both: metrics_frame.h, the arithmetic of the one-clip kernels)
//   mb_kept_energy_kernel  per frame of the compacted signals: frame energies; sized for "no sample removed", a workgroup
//                          at or beyond the device-side kept-frame count exits
// Every value a clip gets depends on that clip's samples only (chunking and summation order are functions of the clip's
// length; no atomics, no cross-clip reductions), so a clip gets the same bits alone, in any batch and in any order.
#include "metrics_frame.h"

#define MB_CHUNK 4096                   // samples per workgroup of the sample-wide stages
#define MB_PER_THREAD (MB_CHUNK / MT)
#define MB_INFO 9                       // int64 per clip: in_off, n, c_off, chunks, f_off, F, kept samples, kept frames, status
#define MB_HEAD 8                       // f64 per clip in the packed output (include/sos_hip.h)
#define MB_FRAMES_PER_WG 4              // frames a workgroup of the frame kernels walks (grid-stride)

// the reference's num_frames = int(n / skip - (winlength / skip)), evaluated in f64 as numpy does and clamped at 0.  NOT
// (n - winlength) / skip in integers: at 22050 Hz (winlength 662, skip 165) n = 21122 gives 123 here and 124 there.
__host__ __device__ static inline int64_t mb_num_frames(int64_t n, int winlength, int skip) {
    const long long f = (long long)((double)n / (double)skip - (double)winlength / (double)skip);
    return f > 0 ? f : 0;
}
__host__ __device__ static inline int64_t mb_num_chunks(int64_t n) { return (n + MB_CHUNK - 1) / MB_CHUNK; }

// info[b] = {in_off, n, c_off, chunks, f_off, F, 0, 0, status}: chunk-indexed arrays start at c_off, frame-indexed ones at
// f_off.  A clip outside the s_cap samples the host summed (ragged_clip_inside), or whose chunks or frames would overrun what
// the host sized from its copy of the lengths, gets status -1 and no work.
__global__ void mb_plan_kernel(const int64_t* __restrict__ offsets, const int64_t* __restrict__ lengths, int nclips, int winlength,
                               int skip, int64_t s_cap, int64_t c_cap, int64_t f_cap, int64_t* __restrict__ info) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t c = 0, f = 0;
    for (int b = 0; b < nclips; ++b) {
        int64_t* ci = info + (int64_t)b * MB_INFO;
        const int64_t n = lengths[b] > 0 ? lengths[b] : 0, off = offsets[b];
        const int64_t chunks = mb_num_chunks(n), F = mb_num_frames(n, winlength, skip);
        const bool ok = ragged_clip_inside(off, n, s_cap) && c + chunks <= c_cap && f + F <= f_cap &&
                        (F == 0 || (F - 1) * skip + winlength <= n);
        ci[0] = ok ? off : 0;
        ci[1] = ok ? n : 0;
        ci[2] = c;
        ci[3] = ok ? chunks : 0;
        ci[4] = f;
        ci[5] = ok ? F : 0;
        ci[6] = 0;
        ci[7] = 0;
        ci[8] = ok ? 0 : -1;
        if (ok) { c += chunks; f += F; }
    }
}

// grid (chunks of the longest clip, clips): part[c_off + chunk] = {sum c^2, sum (c-n)^2, max |c|, sum |n-c|} of the chunk
__global__ __launch_bounds__(MT) void mb_totals_kernel(const float* __restrict__ clean, const float* __restrict__ noisy,
                                                       const int64_t* __restrict__ info, double* __restrict__ part) {
    __shared__ double red[MT];
    const int64_t* ci = info + (int64_t)blockIdx.y * MB_INFO;
    const int64_t in_off = ci[0], n = ci[1], c_off = ci[2], chunks = ci[3];
    if ((int64_t)blockIdx.x >= chunks) return;
    const int64_t i0 = (int64_t)blockIdx.x * MB_CHUNK, i1 = min(n, i0 + MB_CHUNK);
    const float* c = clean + in_off;
    const float* p = noisy + in_off;
    double a = 0, b = 0, m = 0, l = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += MT) {
        const double r = c[i], d = r - (double)p[i];
        a += r * r; b += d * d;
        m = fmax(m, fabs(r));
        l += fabs(d);
    }
    const double sa = block_sum(a, red), sb = block_sum(b, red), sm = block_max(m, red), sl = block_sum(l, red);
    if (threadIdx.x == 0) {
        double* o = part + (c_off + blockIdx.x) * 4;
        o[0] = sa; o[1] = sb; o[2] = sm; o[3] = sl;
    }
}

// one workgroup per clip: head[b] = {sum c^2, sum (c-n)^2, max |c|, sum |n-c|, -, -, frames, status}
__global__ __launch_bounds__(MT) void mb_totals_sum_kernel(const int64_t* __restrict__ info, const double* __restrict__ part,
                                                           double* __restrict__ head) {
    __shared__ double red[MT];
    const int64_t* ci = info + (int64_t)blockIdx.x * MB_INFO;
    const int64_t c_off = ci[2], chunks = ci[3];
    double a = 0, b = 0, m = 0, l = 0;
    for (int64_t k = threadIdx.x; k < chunks; k += MT) {
        const double* o = part + (c_off + k) * 4;
        a += o[0]; b += o[1]; m = fmax(m, o[2]); l += o[3];
    }
    const double sa = block_sum(a, red), sb = block_sum(b, red), sm = block_max(m, red), sl = block_sum(l, red);
    if (threadIdx.x == 0) {
        double* h = head + (int64_t)blockIdx.x * MB_HEAD;
        h[0] = sa; h[1] = sb; h[2] = sm; h[3] = sl;
        h[4] = 0; h[5] = 0;
        h[6] = (double)ci[5];
        h[7] = (double)ci[8];
    }
}

// the silence rule of metrics_ssnr_exclude_silence (:189-199): threshold = float32(max |clean|) * float32(0.03), a sample
// stays when !(|clean| < threshold)
__device__ static inline float mb_threshold(const double* head) { return (float)head[2] * 0.03f; }

// grid (chunks, clips): cnt[c_off + chunk] = kept samples of the chunk
__global__ __launch_bounds__(MT) void mb_keep_count_kernel(const float* __restrict__ clean, const int64_t* __restrict__ info,
                                                           const double* __restrict__ head, int64_t* __restrict__ cnt) {
    __shared__ int scan[MT];
    const int64_t* ci = info + (int64_t)blockIdx.y * MB_INFO;
    const int64_t in_off = ci[0], n = ci[1], c_off = ci[2], chunks = ci[3];
    if ((int64_t)blockIdx.x >= chunks) return;
    const float thr = mb_threshold(head + (int64_t)blockIdx.y * MB_HEAD);
    const int64_t i0 = (int64_t)blockIdx.x * MB_CHUNK, i1 = min(n, i0 + MB_CHUNK);
    const float* c = clean + in_off;
    int k = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += MT) k += !(fabsf(c[i]) < thr) ? 1 : 0;
    const int tot = block_scan_incl(k, scan);
    if (threadIdx.x == MT - 1) cnt[c_off + blockIdx.x] = tot;
}

// one workgroup per clip: cnt[c_off + chunk] becomes the number of kept samples before the chunk (chunked prefix scan: any
// clip length); kept samples k -> info[b][6], head[b][4]; kept frames (the reference's count of k) -> info[b][7], head[b][5]
__global__ __launch_bounds__(MT) void mb_keep_scan_kernel(int64_t* __restrict__ info, int64_t* __restrict__ cnt, int winlength,
                                                          int skip, double* __restrict__ head) {
    __shared__ int scan[MT];
    __shared__ int64_t base;
    int64_t* ci = info + (int64_t)blockIdx.x * MB_INFO;
    const int64_t c_off = ci[2], chunks = ci[3];
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int64_t k0 = 0; k0 < chunks; k0 += MT) {
        const int64_t k = k0 + threadIdx.x;
        const int v = k < chunks ? (int)cnt[c_off + k] : 0;
        const int incl = block_scan_incl(v, scan);
        if (k < chunks) cnt[c_off + k] = base + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) base += scan[MT - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t kf = mb_num_frames(base, winlength, skip);
        ci[6] = base;
        ci[7] = kf;
        head[(int64_t)blockIdx.x * MB_HEAD + 4] = (double)base;
        head[(int64_t)blockIdx.x * MB_HEAD + 5] = (double)kf;
    }
}

// grid (chunks, clips): thread t owns samples [16 t, 16 t + 16) of the chunk; the kept ones of both signals go, in order,
// to oc / op at the clip's offset + kept-before-the-chunk + kept-before-the-thread
__global__ __launch_bounds__(MT) void mb_keep_scatter_kernel(const float* __restrict__ clean, const float* __restrict__ noisy,
                                                             const int64_t* __restrict__ info, const double* __restrict__ head,
                                                             const int64_t* __restrict__ cnt, float* __restrict__ oc,
                                                             float* __restrict__ op) {
    __shared__ int scan[MT];
    const int64_t* ci = info + (int64_t)blockIdx.y * MB_INFO;
    const int64_t in_off = ci[0], n = ci[1], c_off = ci[2], chunks = ci[3];
    if ((int64_t)blockIdx.x >= chunks) return;
    const float thr = mb_threshold(head + (int64_t)blockIdx.y * MB_HEAD);
    const int64_t i0 = (int64_t)blockIdx.x * MB_CHUNK + (int64_t)threadIdx.x * MB_PER_THREAD;
    const float* c = clean + in_off;
    const float* p = noisy + in_off;
    float vc[MB_PER_THREAD];
    unsigned keep = 0;
    int k = 0;
#pragma unroll
    for (int j = 0; j < MB_PER_THREAD; ++j) {
        vc[j] = i0 + j < n ? c[i0 + j] : 0.f;
        if (i0 + j < n && !(fabsf(vc[j]) < thr)) { keep |= 1u << j; ++k; }
    }
    const int incl = block_scan_incl(k, scan);
    int64_t o = in_off + cnt[c_off + blockIdx.x] + (incl - k);
#pragma unroll
    for (int j = 0; j < MB_PER_THREAD; ++j)
        if (keep & (1u << j)) { oc[o] = vc[j]; op[o] = p[i0 + j]; ++o; }
}

// grid (ceil(frames of the longest clip / MB_FRAMES_PER_WG), clips), dynamic LDS 16 winlength bytes (f64 [2][winlength]):
// energy[f_off + f] = {sum (w c)^2, sum (w c - w n)^2} and llr[f_off + f] of every frame of the full signals
__global__ __launch_bounds__(MT) void mb_frames_kernel(const float* __restrict__ clean, const float* __restrict__ noisy,
                                                       const int64_t* __restrict__ info, int winlength, int skip, int P,
                                                       const double* __restrict__ window, double* __restrict__ energy,
                                                       float* __restrict__ llr) {
    extern __shared__ double mb_fr[];
    __shared__ double red[MT];
    __shared__ double R[2][LLR_MAXP + 1];
    const int64_t* ci = info + (int64_t)blockIdx.y * MB_INFO;
    const int64_t in_off = ci[0], f_off = ci[4], F = ci[5];
    for (int64_t f = blockIdx.x; f < F; f += gridDim.x) {
        __syncthreads();                                // lane 0 has left the previous frame's R
        const float* c = clean + in_off + f * skip;
        const float* p = noisy + in_off + f * skip;
        double sa, sb;
        metric_frame_energy(c, p, winlength, window, red, sa, sb);
        if (threadIdx.x == 0) { energy[2 * (f_off + f)] = sa; energy[2 * (f_off + f) + 1] = sb; }
        metric_frame_llr(c, p, winlength, window, P, mb_fr, red, R, llr + f_off + f);
    }
}

// same grid, dynamic LDS (2 winlength + 3 n_fft) * 4 bytes (frames [2][winlength], twiddles [2][n_fft], spectra [n_fft], as
// metric_wss_kernel): wss[f_off + f] of every frame of the full signals; the twiddles are built once per workgroup.  A
// kernel of its own: fused with the LLR it takes 182 VGPRs (two workgroups per CU) instead of 104 (four).
__global__ __launch_bounds__(MT) void mb_wss_kernel(const float* __restrict__ clean, const float* __restrict__ noisy,
                                                    const int64_t* __restrict__ info, int winlength, int skip, int n_fft,
                                                    const double* __restrict__ window, const float* __restrict__ crit, double eps,
                                                    float* __restrict__ wss) {
    extern __shared__ float mb_sm[];
    __shared__ double red[MT];
    __shared__ double en[2][WSS_NCRIT];
    const int64_t* ci = info + (int64_t)blockIdx.y * MB_INFO;
    const int64_t in_off = ci[0], f_off = ci[4], F = ci[5];
    if ((int64_t)blockIdx.x >= F) return;
    float* fc = mb_sm;
    float* fp = fc + winlength;
    float* tc = fp + winlength;
    float* ts = tc + n_fft;
    float* sp = ts + n_fft;
    metric_wss_twiddles(tc, ts, n_fft);
    for (int64_t f = blockIdx.x; f < F; f += gridDim.x) {
        __syncthreads();                                // lane 0 has left the previous frame's band energies
        metric_frame_wss(clean + in_off + f * skip, noisy + in_off + f * skip, winlength, window, n_fft, crit, eps, fc, fp, tc, ts,
                         sp, red, en, wss + f_off + f);
    }
}

// grid as mb_frames_kernel: frame energies of the compacted signals, frames below the device-side kept-frame count only
__global__ __launch_bounds__(MT) void mb_kept_energy_kernel(const float* __restrict__ oc, const float* __restrict__ op,
                                                            const int64_t* __restrict__ info, int winlength, int skip,
                                                            const double* __restrict__ window, double* __restrict__ energy) {
    __shared__ double red[MT];
    const int64_t* ci = info + (int64_t)blockIdx.y * MB_INFO;
    const int64_t in_off = ci[0], f_off = ci[4], KF = min(ci[7], ci[5]);
    for (int64_t f = blockIdx.x; f < KF; f += gridDim.x) {
        double sa, sb;
        metric_frame_energy(oc + in_off + f * skip, op + in_off + f * skip, winlength, window, red, sa, sb);
        if (threadIdx.x == 0) { energy[2 * (f_off + f)] = sa; energy[2 * (f_off + f) + 1] = sb; }
    }
}

namespace {
struct MbLayout {
    int64_t s_total = 0, c_total = 0, f_total = 0, max_c = 0, max_f = 0;
    size_t info = 0, part = 0, cnt = 0, oc = 0, op = 0, bytes = 0;        // workspace
    size_t head = 0, energy = 0, energy_kept = 0, llr = 0, wss = 0, out_bytes = 0;   // packed output
};
MbLayout mb_layout(const int64_t* lengths, int nclips, int winlength, int skip) {
    MbLayout l;
    for (int b = 0; b < nclips; ++b) {
        const int64_t n = lengths[b] > 0 ? lengths[b] : 0, c = mb_num_chunks(n), f = mb_num_frames(n, winlength, skip);
        l.s_total += n; l.c_total += c; l.f_total += f;
        l.max_c = std::max(l.max_c, c);
        l.max_f = std::max(l.max_f, f);
    }
    RaggedBump ws;
    l.info = ws.take((size_t)nclips * MB_INFO * 8);
    l.part = ws.take((size_t)l.c_total * 4 * 8);
    l.cnt = ws.take((size_t)l.c_total * 8);
    l.oc = ws.take((size_t)l.s_total * 4);
    l.op = ws.take((size_t)l.s_total * 4);
    l.bytes = ws.o;
    size_t o = 0;
    l.head = o;        o += (size_t)nclips * MB_HEAD * 8;
    l.energy = o;      o += (size_t)l.f_total * 2 * 8;
    l.energy_kept = o; o += (size_t)l.f_total * 2 * 8;
    l.llr = o;         o += (size_t)l.f_total * 4;
    l.wss = o;         o += (size_t)l.f_total * 4;
    l.out_bytes = o;
    return l;
}
bool mb_args_ok(const int64_t* lengths, int nclips, int winlength, int skip, int n_fft) {
    return ragged_clips_ok(lengths, nclips) && winlength > 0 && skip > 0 && n_fft >= 2 * winlength && (n_fft & (n_fft - 1)) == 0;
}
size_t mb_frame_lds(int winlength, int n_fft) { return ((size_t)2 * winlength + 3 * (size_t)n_fft) * 4; }
}  // namespace

extern "C" int64_t sos_metric_batch_workspace_bytes(const int64_t* lengths, int nclips, int winlength, int skip, int n_fft) {
    if (!mb_args_ok(lengths, nclips, winlength, skip, n_fft)) {
        sos_set_error("sos_metric_batch_workspace_bytes: bad args");
        return -1;
    }
    return (int64_t)std::max<size_t>(mb_layout(lengths, nclips, winlength, skip).bytes, 256);
}

extern "C" int sos_metric_batch(const float* clean, const float* noisy, const int64_t* offsets, const int64_t* lengths,
                                const int64_t* lengths_host, int nclips, int winlength, int skip, int n_fft, int P,
                                const double* window, const float* crit_filter, double eps, void* workspace,
                                int64_t workspace_bytes, void* out, int64_t out_bytes, sos_stream_t stream) {
    if (!clean || !noisy || !offsets || !lengths || !window || !crit_filter || !workspace || !out ||
        !mb_args_ok(lengths_host, nclips, winlength, skip, n_fft) || P < 1 || P > LLR_MAXP || P >= winlength) {
        sos_set_error("sos_metric_batch: bad args");
        return SOS_EINVAL;
    }
    const size_t lds = mb_frame_lds(winlength, n_fft);
    if (lds > 60 * 1024) {
        sos_set_error("sos_metric_batch: winlength %d with n_fft %d needs %lld bytes of LDS per frame, 61440 is the limit", winlength,
                      n_fft, (long long)lds);
        return SOS_EINVAL;
    }
    const MbLayout l = mb_layout(lengths_host, nclips, winlength, skip);
    if (workspace_bytes < (int64_t)l.bytes || out_bytes < (int64_t)l.out_bytes) {
        sos_set_error("sos_metric_batch: workspace of %lld bytes (%lld needed), output of %lld bytes (%lld needed)",
                      (long long)workspace_bytes, (long long)l.bytes, (long long)out_bytes, (long long)l.out_bytes);
        return SOS_EINVAL;
    }
    char* ws = (char*)workspace;
    int64_t* info = (int64_t*)(ws + l.info);
    double* part = (double*)(ws + l.part);
    int64_t* cnt = (int64_t*)(ws + l.cnt);
    float* oc = (float*)(ws + l.oc);
    float* op = (float*)(ws + l.op);
    char* ob = (char*)out;
    double* head = (double*)(ob + l.head);
    double* energy = (double*)(ob + l.energy);
    double* energy_kept = (double*)(ob + l.energy_kept);
    float* llr = (float*)(ob + l.llr);
    float* wss = (float*)(ob + l.wss);
    hipStream_t s = (hipStream_t)stream;
    const dim3 chunk_grid(ragged_grid(l.max_c, 1, 0x7fffffff), nclips);
    const dim3 frame_grid(ragged_grid(l.max_f, MB_FRAMES_PER_WG, 0x7fffffff), nclips);
    int rc;
    hipLaunchKernelGGL(mb_plan_kernel, dim3(1), dim3(64), 0, s, offsets, lengths, nclips, winlength, skip, l.s_total, l.c_total,
                       l.f_total, info);
    if ((rc = sos_check_launch("sos_metric_batch: plan")) != SOS_OK) return rc;
    hipLaunchKernelGGL(mb_totals_kernel, chunk_grid, dim3(MT), 0, s, clean, noisy, info, part);
    if ((rc = sos_check_launch("sos_metric_batch: totals")) != SOS_OK) return rc;
    hipLaunchKernelGGL(mb_totals_sum_kernel, dim3(nclips), dim3(MT), 0, s, info, part, head);
    if ((rc = sos_check_launch("sos_metric_batch: totals sum")) != SOS_OK) return rc;
    hipLaunchKernelGGL(mb_keep_count_kernel, chunk_grid, dim3(MT), 0, s, clean, info, head, cnt);
    if ((rc = sos_check_launch("sos_metric_batch: keep count")) != SOS_OK) return rc;
    hipLaunchKernelGGL(mb_keep_scan_kernel, dim3(nclips), dim3(MT), 0, s, info, cnt, winlength, skip, head);
    if ((rc = sos_check_launch("sos_metric_batch: keep scan")) != SOS_OK) return rc;
    hipLaunchKernelGGL(mb_keep_scatter_kernel, chunk_grid, dim3(MT), 0, s, clean, noisy, info, head, cnt, oc, op);
    if ((rc = sos_check_launch("sos_metric_batch: keep scatter")) != SOS_OK) return rc;
    if (l.max_f > 0) {
        hipLaunchKernelGGL(mb_frames_kernel, frame_grid, dim3(MT), (size_t)winlength * 16, s, clean, noisy, info, winlength, skip, P,
                           window, energy, llr);
        if ((rc = sos_check_launch("sos_metric_batch: frames")) != SOS_OK) return rc;
        hipLaunchKernelGGL(mb_wss_kernel, frame_grid, dim3(MT), lds, s, clean, noisy, info, winlength, skip, n_fft, window,
                           crit_filter, eps, wss);
        if ((rc = sos_check_launch("sos_metric_batch: wss")) != SOS_OK) return rc;
        hipLaunchKernelGGL(mb_kept_energy_kernel, frame_grid, dim3(MT), 0, s, oc, op, info, winlength, skip, window, energy_kept);
        if ((rc = sos_check_launch("sos_metric_batch: kept energy")) != SOS_OK) return rc;
    }
    return SOS_OK;
}
