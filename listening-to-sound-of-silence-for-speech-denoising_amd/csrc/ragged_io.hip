// ragged_io.hip -- the two copies between "clips back to back in one buffer" (what audio_io.load_batch_device / torch.cat
// produce and what one download wants) and "one padded row per clip" (what the STFT, the networks and the ISTFT take), each
// in ONE launch whatever the number of clips:
//   ragged_stage_kernel   clips (+ per-clip frame decisions and ratio) -> wave (B, stride), masked (B, stride), mask back to back
//   ragged_unpack_kernel  padded rows (R, stride) + {row, valid, out offset} -> one back-to-back buffer
// Pure streaming.  A thread handles four consecutive samples of a row: the row side is one 16-byte access when the stride is
// a multiple of four samples, the back-to-back side when the clip starts on a 16-byte boundary and the four samples are all
// inside the clip; scalar accesses otherwise (the two sides of an unaligned clip cannot both be aligned).
// The mask is mask_sample of mask_rule.h, the rule of sos_bits_to_mask: a clip's bits are those of
// sos_bits_to_mask(bits, 1, frames, ratio, samples) for that clip alone, in any group and any order.
// Bounds: the rule of ragged.h -- the host refuses a table entry outside the samples / frames it summed from table_host
// (SOS_EINVAL), the kernels skip an entry of the DEVICE table that fails the same rule.
#include "ragged.h"
#include "mask_rule.h"

#define RIO_THREADS 256
#define RIO_MAX_GRID 1024               // workgroups along a row (they stride over what the grid does not cover)
#define RIO_UNPACK_COLS 3               // int64 per entry: row, valid samples, output offset

__global__ __launch_bounds__(RIO_THREADS) void ragged_stage_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ table, int64_t total, const uint8_t* __restrict__ bits,
    int64_t total_bits, const double* __restrict__ ratios, int64_t stride, float* __restrict__ wave, float* __restrict__ masked,
    float* __restrict__ mask) {
    const int64_t b = blockIdx.y;
    const RaggedClip c = ragged_clip(table, b);
    const int64_t off = c.off, n = c.n, boff = c.foff, nfr = c.frames;
    if (n > stride || !(bits ? ragged_row_inside(c, total, total_bits) : ragged_clip_inside(off, n, total))) return;
    const double ratio = bits ? ratios[b] : 0.0;
    if (bits && !(ratio > 1.0)) return;
    const float* xc = x + off;
    const uint8_t* bc = bits ? bits + boff : nullptr;
    float* wrow = wave + b * stride;
    float* mrow = bits ? masked + b * stride : nullptr;
    float* mc = bits ? mask + off : nullptr;
    const bool row_vec = (stride & 3) == 0 && ragged_aligned16(wave) && ragged_aligned16(masked);
    const bool clip_vec = ragged_aligned16(xc) && ragged_aligned16(mc);
    for (int64_t j0 = ((int64_t)blockIdx.x * RIO_THREADS + threadIdx.x) * 4; j0 < stride; j0 += (int64_t)gridDim.x * RIO_THREADS * 4) {
        const bool full = j0 + 4 <= n;                       // all four samples inside the clip
        float v[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f};
        ragged_load4(xc, j0, n, full && clip_vec, v);
        if (bits) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < n) m[k] = mask_sample(bc, nfr, ratio, n, j0 + k);
            ragged_store4(mc, j0, n, full && clip_vec, m);
        }
        // the rows: zero from the clip's end to the stride (v and m are 0 there); row_vec: the stride is a multiple of four,
        // so j0 + 4 <= stride
        ragged_store4(wrow, j0, stride, row_vec, v);
        if (bits) {
            const float vm[4] = {v[0] * m[0], v[1] * m[1], v[2] * m[2], v[3] * m[3]};
            ragged_store4(mrow, j0, stride, row_vec, vm);
        }
    }
}

__global__ __launch_bounds__(RIO_THREADS) void ragged_unpack_kernel(const float* __restrict__ rows, int64_t n_rows, int64_t stride,
                                                                   const int64_t* __restrict__ table, int64_t total,
                                                                   float* __restrict__ out) {
    const int64_t* te = table + (int64_t)blockIdx.y * RIO_UNPACK_COLS;
    const int64_t row = te[0], n = te[1], off = te[2];
    if (row < 0 || row >= n_rows || n > stride || !ragged_clip_inside(off, n, total)) return;
    const float* src = rows + row * stride;
    float* dst = out + off;
    const bool row_vec = (stride & 3) == 0 && ragged_aligned16(rows), out_vec = ragged_aligned16(dst);
    for (int64_t j0 = ((int64_t)blockIdx.x * RIO_THREADS + threadIdx.x) * 4; j0 < n; j0 += (int64_t)gridDim.x * RIO_THREADS * 4) {
        const bool full = j0 + 4 <= n;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        ragged_load4(src, j0, n, full && row_vec, v);
        ragged_store4(dst, j0, n, full && out_vec, v);
    }
}

extern "C" int sos_ragged_stage_f32(const float* x, const int64_t* table, const int64_t* table_host, int nclips,
                                    const uint8_t* bits, const double* ratios, const double* ratios_host, int64_t stride,
                                    float* wave, float* masked, float* mask, sos_stream_t stream) {
    if (!x || !table || !wave) { sos_set_error("sos_ragged_stage_f32: null pointer"); return SOS_EINVAL; }
    if (!ragged_clips_ok(table_host, nclips) || stride < 1 || stride > INT64_MAX / 8 / RAGGED_MAX_CLIPS) {
        sos_set_error("sos_ragged_stage_f32: bad args (1 .. 65535 clips, got %d; stride %lld)", nclips, (long long)stride);
        return SOS_EINVAL;
    }
    if (bits && (!ratios || !ratios_host || !masked || !mask)) {
        sos_set_error("sos_ragged_stage_f32: frame decisions need ratios, ratios_host, masked and mask");
        return SOS_EINVAL;
    }
    RaggedSum ns, nf;
    int bad = std::min(ragged_sum_column(table_host, nclips, RAGGED_CLIP_COLS, 1, 0, stride, &ns),
                       ragged_sum_column(table_host, nclips, RAGGED_CLIP_COLS, 3, 0, INT64_MAX, &nf));
    if (bad < nclips) {
        const RaggedClip c = ragged_clip(table_host, bad);
        sos_set_error("sos_ragged_stage_f32: clip %d has %lld samples (stride %lld) and %lld frames", bad, (long long)c.n,
                      (long long)stride, (long long)c.frames);
        return SOS_EINVAL;
    }
    bad = ragged_first_outside(table_host, nclips, RAGGED_CLIP_COLS, 0, 1, ns.total);
    if (bits) bad = std::min(bad, ragged_first_outside(table_host, nclips, RAGGED_CLIP_COLS, 2, 3, nf.total));
    for (int b = 0; bits && b < bad; ++b)                    // the clips before the first that lies outside
        if (!(ratios_host[b] > 1.0)) {
            sos_set_error("sos_ragged_stage_f32: clip %d has ratio %g (samples per frame must exceed 1)", b, ratios_host[b]);
            return SOS_EINVAL;
        }
    if (bad < nclips) {
        const RaggedClip c = ragged_clip(table_host, bad);
        sos_set_error("sos_ragged_stage_f32: clip %d (samples %lld + %lld, frames %lld + %lld) lies outside the %lld samples / "
                      "%lld frames of the table", bad, (long long)c.off, (long long)c.n, (long long)c.foff, (long long)c.frames,
                      (long long)ns.total, (long long)nf.total);
        return SOS_EINVAL;
    }
    const dim3 grid(ragged_grid((stride + 3) / 4, RIO_THREADS, RIO_MAX_GRID), (unsigned)nclips);
    hipLaunchKernelGGL(ragged_stage_kernel, grid, dim3(RIO_THREADS), 0, (hipStream_t)stream, x, table, ns.total, bits, nf.total,
                       ratios, stride, wave, masked, mask);
    return sos_check_launch("sos_ragged_stage_f32");
}

extern "C" int sos_ragged_unpack_f32(const float* rows, int64_t n_rows, int64_t stride, const int64_t* table,
                                     const int64_t* table_host, int nentries, float* out, sos_stream_t stream) {
    if (!rows || !table || !out) { sos_set_error("sos_ragged_unpack_f32: null pointer"); return SOS_EINVAL; }
    if (!ragged_clips_ok(table_host, nentries) || n_rows < 1 || stride < 1 || n_rows > INT64_MAX / 8 / stride) {
        sos_set_error("sos_ragged_unpack_f32: bad args (1 .. 65535 entries, got %d; %lld rows of %lld)", nentries, (long long)n_rows,
                      (long long)stride);
        return SOS_EINVAL;
    }
    RaggedSum ns;
    int bad = ragged_sum_column(table_host, nentries, RIO_UNPACK_COLS, 1, 0, stride, &ns);
    for (int e = 0; e < bad; ++e)                            // the entries before it name a row there is
        if (table_host[e * RIO_UNPACK_COLS] < 0 || table_host[e * RIO_UNPACK_COLS] >= n_rows) bad = e;
    if (bad < nentries) {
        const int64_t* te = table_host + bad * RIO_UNPACK_COLS;
        sos_set_error("sos_ragged_unpack_f32: entry %d takes %lld samples of row %lld (%lld rows of %lld)", bad, (long long)te[1],
                      (long long)te[0], (long long)n_rows, (long long)stride);
        return SOS_EINVAL;
    }
    bad = ragged_first_outside(table_host, nentries, RIO_UNPACK_COLS, 2, 1, ns.total);
    if (bad < nentries) {
        const int64_t* te = table_host + bad * RIO_UNPACK_COLS;
        sos_set_error("sos_ragged_unpack_f32: entry %d (output %lld + %lld) lies outside the %lld samples of the table", bad,
                      (long long)te[2], (long long)te[1], (long long)ns.total);
        return SOS_EINVAL;
    }
    const dim3 grid(ragged_grid((ns.longest + 3) / 4, RIO_THREADS, RIO_MAX_GRID), (unsigned)nentries);
    hipLaunchKernelGGL(ragged_unpack_kernel, grid, dim3(RIO_THREADS), 0, (hipStream_t)stream, rows, n_rows, stride, table, ns.total,
                       out);
    return sos_check_launch("sos_ragged_unpack_f32");
}
