// silence_label.hip -- ground-truth silent-interval labels of clean speech for a ragged batch of clips: per video frame an
// energy, a threshold relative to the clip's loudest frame and two run-length rules (float64 restatement:
// tests/silence_reference.py; parity with the reference's preprocessing/get_bitstream_better is unpinned).  One batch is two
// launches without host synchronisation:
//   silence_energy_kernel  E[i] = mean x^2 over frame i = samples [int(i r), min(int((i+1) r), n)), r = sr / fps.  A wave per
//                          frame; lane l takes the samples 4k .. 4k+3 (counted from the frame's start) of every k = l mod 64
//                          in rising k, one 16-byte load each (frames start on any sample: the load asks for 4-byte
//                          alignment only), the last partial group sample by sample; f64 FMAs, then the 64 lanes by butterfly.
//                          Which lane adds which sample depends on the sample's place in its frame only, so E has the same
//                          bits wherever the clip lies in the buffer.  Every sample is read once.
//   silence_label_kernel   one workgroup per clip: max E, T = max(rel max E, floor), quiet = E <= T; then twice "the runs of
//                          the sequence" (a boundary scan over tiles of 256 frames, the run count carried across tiles, every
//                          frame's run number and every run's first frame into the workspace) and a rule over the runs as
//                          they were when the pass began: 1. a non-quiet run shorter than min_speech with a quiet run on both
//                          sides turns quiet, 2. a quiet run shorter than min_silent turns non-quiet.
// bits (1 = non-silent, the convention of sos_bits_to_mask) and E lie back to back at the frame offsets of the table, the
// clip rows of ragged.h (sos_ragged_stage_f32 takes the same).  No atomics; a clip's bits depend on that clip's samples only.
// Bounds: the rule of ragged.h -- the host refuses a table entry outside the samples / frames it summed from table_host; the
// kernels follow the DEVICE table and parameters and give a clip that fails the same rules (ragged_row_inside, sl_frames_fit)
// status -1 and no work; every frame's sample range is clamped to its clip.  Frame edges: frame_edge of mask_rule.h, the mask's.
#include "ragged.h"
#include "mask_rule.h"

#define SL_PARAMS 5                     // f64 per clip: ratio, rel, floor, min_silent, min_speech
#define SL_OUT 6                        // f64 per clip: max E, T, silent frames, silent runs, frames, status
#define SL_WAVES (MT / 64)              // frames a workgroup of the energy kernel works on at a time
#define SL_MAX_GRID 4096                // workgroups along a clip's frames (they stride over what the grid does not cover)
#define SL_MAX_FRAMES 2147483000LL      // frame numbers and run numbers are int32 in the workspace
#define SL_MAX_RATIO 2147483648.0       // frames x ratio stays inside int64

typedef float sl_f32x4 __attribute__((ext_vector_type(4)));
typedef sl_f32x4 sl_f32x4_u __attribute__((aligned(4)));             // four consecutive samples at any sample address

__host__ __device__ static inline bool sl_ratio_ok(double ratio) { return ratio > 1.0 && ratio <= SL_MAX_RATIO; }

// `frames` frames of `ratio` samples tile a clip of n samples: none is empty and no sample is left over
__host__ __device__ static inline bool sl_frames_fit(int64_t n, int64_t frames, double ratio) {
    return n >= 1 && frames >= 1 && frames <= SL_MAX_FRAMES && frame_edge(frames - 1, ratio) < n && n <= frame_edge(frames, ratio);
}

__host__ __device__ static inline bool sl_params_ok(const double* p) {
    return sl_ratio_ok(p[0]) && p[1] >= 0.0 && p[2] >= 0.0 && p[3] >= 1.0 && p[4] >= 1.0;
}

// what both kernels ask of a clip of the device table before they touch anything
__device__ static inline bool sl_clip_ok(const RaggedClip& c, const double* p, int64_t total, int64_t total_frames) {
    return ragged_row_inside(c, total, total_frames) && sl_params_ok(p) && sl_frames_fit(c.n, c.frames, p[0]);
}

__global__ __launch_bounds__(MT) void silence_energy_kernel(const float* __restrict__ x, const int64_t* __restrict__ table,
                                                            const double* __restrict__ params, int64_t total, int64_t total_frames,
                                                            double* __restrict__ energy) {
    const RaggedClip c = ragged_clip(table, blockIdx.y);
    const double* p = params + (int64_t)blockIdx.y * SL_PARAMS;
    if (!sl_clip_ok(c, p, total, total_frames)) return;
    const int64_t n = c.n, frames = c.frames;
    const double ratio = p[0];
    const float* xc = x + c.off;
    double* ec = energy + c.foff;
    const int lane = threadIdx.x & 63;
    for (int64_t f = (int64_t)blockIdx.x * SL_WAVES + (threadIdx.x >> 6); f < frames; f += (int64_t)gridDim.x * SL_WAVES) {
        // clamped to the clip, whatever the ratio: 0 <= lo <= hi <= n
        const int64_t lo = min(max(frame_edge(f, ratio), (int64_t)0), n), hi = min(max(frame_edge(f + 1, ratio), lo), n);
        const int64_t len = hi - lo, groups = len >> 2;
        const float* xf = xc + lo;
        double acc = 0.0;
        int64_t k = lane;
        for (; k + 192 < groups; k += 256) {                              // four loads in flight, added in rising k
            const sl_f32x4 a = *(const sl_f32x4_u*)(xf + 4 * k), b = *(const sl_f32x4_u*)(xf + 4 * (k + 64));
            const sl_f32x4 c = *(const sl_f32x4_u*)(xf + 4 * (k + 128)), d = *(const sl_f32x4_u*)(xf + 4 * (k + 192));
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = fma((double)a[j], (double)a[j], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = fma((double)b[j], (double)b[j], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = fma((double)c[j], (double)c[j], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = fma((double)d[j], (double)d[j], acc);
        }
        for (; k < groups; k += 64) {
            const sl_f32x4 a = *(const sl_f32x4_u*)(xf + 4 * k);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = fma((double)a[j], (double)a[j], acc);
        }
        if (k == groups)                                                 // the lane whose turn the partial group is
            for (int64_t t = 4 * groups; t < len; ++t) acc = fma((double)xf[t], (double)xf[t], acc);
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) ec[f] = len > 0 ? acc / (double)len : 0.0;
    }
}

// The runs of q(0 .. frames): rid[i] = number of the run frame i lies in, rs[r] = first frame of run r, rs[runs] = frames.
// Returns the number of runs (the same in every thread).  Ends on a barrier: rid / rs are visible to the workgroup.
template <class Q>
__device__ static inline int sl_build_runs(Q q, int frames, int* __restrict__ rid, int* __restrict__ rs, int* scan) {
    int carry = 0;
    for (int base = 0; base < frames; base += MT) {
        const int i = base + (int)threadIdx.x;
        const bool in = i < frames;
        const int b = in && (i == 0 || q(i) != q(i - 1)) ? 1 : 0;
        const int incl = block_scan_incl(b, scan);
        const int tile = scan[MT - 1];
        if (in) {
            rid[i] = carry + incl - 1;
            if (b) rs[carry + incl - 1] = i;
        }
        carry += tile;
        __syncthreads();                                                 // scan[MT - 1] read before the next tile's scan
    }
    if (threadIdx.x == 0) rs[carry] = frames;
    __syncthreads();
    return carry;
}

__global__ __launch_bounds__(MT) void silence_label_kernel(const int64_t* __restrict__ table, const double* __restrict__ params,
                                                           int64_t total, int64_t total_frames, const double* __restrict__ energy,
                                                           int* __restrict__ rid_all, int* __restrict__ rs_all,
                                                           uint8_t* __restrict__ bits, double* __restrict__ out) {
    __shared__ double red[MT];
    __shared__ int scan[MT];
    const RaggedClip c = ragged_clip(table, blockIdx.x);
    const double* p = params + (int64_t)blockIdx.x * SL_PARAMS;
    double* o = out + (int64_t)blockIdx.x * SL_OUT;
    if (!sl_clip_ok(c, p, total, total_frames)) {
        if (threadIdx.x == 0) { o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0; o[4] = -1.0; o[5] = -1.0; }
        return;
    }
    const int frames = (int)c.frames;
    const double* ec = energy + c.foff;
    uint8_t* bc = bits + c.foff;
    int* rid = rid_all + c.foff;
    int* rs = rs_all + c.foff + blockIdx.x;                              // frames + 1 entries per clip
    const double rel = p[1], floor_ = p[2], min_silent = p[3], min_speech = p[4];
    double m = 0.0;                                                      // energies are >= 0
    for (int i = threadIdx.x; i < frames; i += MT) m = fmax(m, ec[i]);
    const double emax = block_max(m, red);
    const double T = fmax(__dmul_rn(rel, emax), floor_);
    // pass 1 over the runs of the raw decision; bc holds "quiet" until the last step
    int runs = sl_build_runs([&](int i) { return ec[i] <= T ? 1 : 0; }, frames, rid, rs, scan);
    for (int i = threadIdx.x; i < frames; i += MT) {
        const int r = min(max(rid[i], 0), runs - 1);                     // (a run number of this clip unless device entries overlap)
        int q = ec[i] <= T ? 1 : 0;
        if (!q && r > 0 && r < runs - 1 && (double)(rs[r + 1] - rs[r]) < min_speech) q = 1;
        bc[i] = (uint8_t)q;
    }
    __syncthreads();                                                     // bc written, rid / rs read
    // pass 2 over the runs as pass 1 left them
    runs = sl_build_runs([&](int i) { return (int)bc[i]; }, frames, rid, rs, scan);
    double n_silent = 0.0, n_runs = 0.0;
    for (int i = threadIdx.x; i < frames; i += MT) {
        const int r = min(max(rid[i], 0), runs - 1);
        int q = bc[i];
        if (q && (double)(rs[r + 1] - rs[r]) < min_silent) q = 0;
        n_silent += q;
        n_runs += q && rs[r] == i ? 1 : 0;                               // kept quiet runs stay apart: one per first frame
        bc[i] = (uint8_t)(1 - q);
    }
    const double s0 = block_sum(n_silent, red), s1 = block_sum(n_runs, red);          // integers: exact
    if (threadIdx.x == 0) { o[0] = emax; o[1] = T; o[2] = s0; o[3] = s1; o[4] = (double)frames; o[5] = 0.0; }
}

// the workspace: a run number per frame at 0, then frames + 1 run starts per clip at sl_rs, each array to 256 bytes
static size_t sl_rs(int64_t frames) { return align256((size_t)frames * 4); }
static size_t sl_bytes(int64_t frames, int nclips) { return sl_rs(frames) + align256(((size_t)frames + (size_t)nclips) * 4); }

extern "C" int64_t sos_silence_label_workspace_bytes(const int64_t* table_host, int nclips) {
    if (!ragged_clips_ok(table_host, nclips)) {
        sos_set_error("sos_silence_label_workspace_bytes: bad args (1 .. 65535 clips, got %d)", nclips);
        return -1;
    }
    RaggedSum nf;                                                        // a clip the launch would refuse by name counts as 0
    for (int b = 0; b < nclips; ++b) b = ragged_sum_column(table_host, nclips, RAGGED_CLIP_COLS, 3, 1, SL_MAX_FRAMES, &nf, b);
    return (int64_t)sl_bytes(nf.total, nclips);
}

extern "C" int sos_silence_label_batch(const float* x, const int64_t* table, const int64_t* table_host, int nclips,
                                       const double* params, const double* params_host, void* workspace,
                                       int64_t workspace_bytes, uint8_t* bits, double* energy, double* out, sos_stream_t stream) {
    if (!x || !table || !table_host || !params || !params_host || !workspace || !bits || !energy || !out) {
        sos_set_error("sos_silence_label_batch: null pointer");
        return SOS_EINVAL;
    }
    if (!ragged_clips_ok(table_host, nclips)) {
        sos_set_error("sos_silence_label_batch: bad args (1 .. 65535 clips, got %d)", nclips);
        return SOS_EINVAL;
    }
    RaggedSum ns, nf;
    int bad = std::min(ragged_sum_column(table_host, nclips, RAGGED_CLIP_COLS, 1, 1, INT64_MAX, &ns),
                       ragged_sum_column(table_host, nclips, RAGGED_CLIP_COLS, 3, 1, SL_MAX_FRAMES, &nf));
    if (bad < nclips) {
        const RaggedClip c = ragged_clip(table_host, bad);
        sos_set_error("sos_silence_label_batch: clip %d has %lld samples and %lld frames (at least 1 of each)", bad, (long long)c.n,
                      (long long)c.frames);
        return SOS_EINVAL;
    }
    bad = std::min(ragged_first_outside(table_host, nclips, RAGGED_CLIP_COLS, 0, 1, ns.total),
                   ragged_first_outside(table_host, nclips, RAGGED_CLIP_COLS, 2, 3, nf.total));
    for (int b = 0; b < nclips; ++b) {
        const RaggedClip c = ragged_clip(table_host, b);
        const double* p = params_host + b * SL_PARAMS;
        if (b == bad) {
            sos_set_error("sos_silence_label_batch: clip %d (samples %lld + %lld, frames %lld + %lld) lies outside the %lld samples / "
                          "%lld frames of the table", b, (long long)c.off, (long long)c.n, (long long)c.foff, (long long)c.frames,
                          (long long)ns.total, (long long)nf.total);
            return SOS_EINVAL;
        }
        if (!sl_ratio_ok(p[0])) {
            sos_set_error("sos_silence_label_batch: clip %d has ratio %g (samples per frame must exceed 1)", b, p[0]);
            return SOS_EINVAL;
        }
        if (!(p[3] >= 1.0) || !(p[4] >= 1.0)) {
            sos_set_error("sos_silence_label_batch: clip %d has minimum run lengths %g (silent) and %g (speech); both must be at "
                          "least 1 frame", b, p[3], p[4]);
            return SOS_EINVAL;
        }
        if (!(p[1] >= 0.0) || !(p[2] >= 0.0)) {
            sos_set_error("sos_silence_label_batch: clip %d has relative threshold %g and floor %g (neither may be negative)", b, p[1],
                          p[2]);
            return SOS_EINVAL;
        }
        if (!sl_frames_fit(c.n, c.frames, p[0])) {
            sos_set_error("sos_silence_label_batch: clip %d: %lld frames of %g samples do not tile %lld samples (%s)", b,
                          (long long)c.frames, p[0], (long long)c.n,
                          frame_edge(c.frames - 1, p[0]) >= c.n ? "the last frame would be empty" : "samples would be left over");
            return SOS_EINVAL;
        }
    }
    const int64_t need = (int64_t)sl_bytes(nf.total, nclips);
    if (workspace_bytes < need) {
        sos_set_error("sos_silence_label_batch: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
        return SOS_ENOSPC;
    }
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    hipLaunchKernelGGL(silence_energy_kernel, dim3(ragged_grid(nf.longest, SL_WAVES, SL_MAX_GRID), (unsigned)nclips), dim3(MT), 0, s,
                       x, table, params, ns.total, nf.total, energy);
    if ((rc = sos_check_launch("sos_silence_label_batch: energies")) != SOS_OK) return rc;
    hipLaunchKernelGGL(silence_label_kernel, dim3((unsigned)nclips), dim3(MT), 0, s, table, params, ns.total, nf.total,
                       (const double*)energy, (int*)ws, (int*)(ws + sl_rs(nf.total)), bits, out);
    return sos_check_launch("sos_silence_label_batch: labels");
}
