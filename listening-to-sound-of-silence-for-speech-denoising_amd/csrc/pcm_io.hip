// pcm_io.hip -- the two copies between "WAVE data as the file holds it" and "one f32 plane per channel", each for a group of
// files in ONE launch (audio_io.decode_planes_batch_device / encode_batch_device; float64 restatement: tests/pcm_reference.py):
//   pcm_planes_kernel   interleaved [frames][channels] samples of one format, files back to back -> f32 channel planes
//   pcm_encode_kernel   f32 channel planes -> interleaved s16 / packed s24 / s32 / u8 / f32, files back to back, plus the
//                       number of samples per file that saturated or were NaN
// Pure streaming, no reuse: every input sample is read once, every output byte written once.  A thread takes four consecutive
// INTERLEAVED elements, so adjacent lanes cover adjacent elements of the interleaved side: one 4 * width byte access where the
// file's first element lies on such a boundary, element by element otherwise.  The plane side is one 16-byte access for a
// one-channel file whose plane is aligned, scalar otherwise (four interleaved elements of a c-channel file lie c planes apart).
// Which access is taken changes no value.  Packed s24 is written as absolute dwords: a thread owns three aligned dwords = twelve
// bytes of the file's byte range wherever the file starts, and only the threads at the two ends of a file store single bytes.
// G.711 (A-law / mu-law code bytes, sos_g711_planes_batch_f32 / sos_g711_encode_batch) is two more sample types of the same two
// kernels: four codes are one dword, and the plane side is the template's.
// Dither (sos_pcm_encode_dither_batch; the rule: dither_core.h) is a template parameter of the two encode kernels: kind 0 is the
// kernel without it, instruction for instruction; kinds 1 / 2 draw every sample's dither from a counter-based generator inside
// the kernel, keyed by (seed, file key, channel, absolute frame).  A one-channel thread's four frames are one or two Philox
// blocks; a stereo thread visits its two channels in turn (two frames each: one or two blocks per channel); three and more
// channels take one block per element.
// Bounds: the rule of ragged.h -- the host refuses a row of table_host outside the elements it summed (SOS_EINVAL), the kernels
// skip a row of the DEVICE table that fails the same rule.
#include "ragged.h"
#include "pcm_core.h"
#include "dither_core.h"

#define PIO_THREADS 256
#define PIO_MAX_GRID 1024               // workgroups along a file (they stride over what the grid does not cover)
#define PIO_MAX_CHANNELS 64
#define PIO_PLANES_COLS 4               // int64 per file: pcm element offset, frames, channels, first output sample
#define PIO_ENCODE_COLS 5               // int64 per file: first plane sample, plane length, channels, frames, output element offset
#define PIO_DITHER_COLS 7               // the same, then the file's dither key and the absolute frame of its first frame

// `n` rows of `ch` channels starting at `off` lie inside `total` elements (no overflowing multiply)
__host__ __device__ static inline bool pio_inside(int64_t off, int64_t n, int64_t ch, int64_t total) {
    return ch >= 1 && ch <= PIO_MAX_CHANNELS && n >= 0 && n <= total / ch && ragged_clip_inside(off, n * ch, total);
}

template <typename T> struct alignas(4 * sizeof(T)) PioVec4 { T v[4]; };

template <typename T>
__global__ __launch_bounds__(PIO_THREADS) void pcm_planes_kernel(const T* __restrict__ pcm, const int64_t* __restrict__ table,
                                                                 int64_t total, float* __restrict__ out) {
    const int64_t* te = table + (int64_t)blockIdx.y * PIO_PLANES_COLS;
    const int64_t off = te[0], frames = te[1], ch = te[2], ooff = te[3];
    if (!pio_inside(off, frames, ch, total) || !pio_inside(ooff, frames, ch, total)) return;
    const int64_t n = frames * ch;
    const T* src = pcm + off;
    float* dst = out + ooff;
    const bool src_vec = ((uintptr_t)src & (4 * sizeof(T) - 1)) == 0;
    const bool dst_vec = ch == 1 && ragged_aligned16(dst);
    for (int64_t e0 = ((int64_t)blockIdx.x * PIO_THREADS + threadIdx.x) * 4; e0 < n; e0 += (int64_t)gridDim.x * PIO_THREADS * 4) {
        const bool full = e0 + 4 <= n;
        T s[4] = {};
        if (full && src_vec) {
            const PioVec4<T> q = *(const PioVec4<T>*)(src + e0);
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = q.v[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < n) s[k] = src[e0 + k];
        }
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = Pcm<T>::cvt(s[k]);
        if (ch == 1) {
            ragged_store4(dst, e0, n, full && dst_vec, v);
        } else {
            int64_t i = e0 / ch, c = e0 - i * ch;             // frame and channel of the first element
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e0 + k < n) dst[c * frames + i] = v[k];
                if (++c == ch) { c = 0; ++i; }
            }
        }
    }
}

// ---- encode.  The rule (include/sos_hip.h): q = rint(x * S) half to even in double (a float times a power of two is exact
// there), NaN -> 0 and counted, saturated to [-S, S - 1] and counted when that changed it.
template <int BITS>
__device__ __forceinline__ int32_t pio_round(double d, int& clipped) {
    const double S = (double)((int64_t)1 << (BITS - 1));
    const double r = rint(d);
    const bool nan = d != d, hi = r > S - 1.0, lo = r < -S;  // selects, no branches (rint(NaN) compares false twice)
    clipped += (int)(nan | hi | lo);
    const double q = nan ? 0.0 : hi ? S - 1.0 : lo ? -S : r;
    return (int32_t)q;                                       // |q| <= 2^31: one v_cvt_i32_f64
}
template <int BITS>
__device__ __forceinline__ int32_t pio_quantise(float x, int& clipped) {
    return pio_round<BITS>((double)x * (double)((int64_t)1 << (BITS - 1)), clipped);
}
// with a dither of d16 / 65536 LSB (dither_core.h): added in double before the one rounding; counted after it
template <int BITS>
__device__ __forceinline__ int32_t pio_quantise(float x, int32_t d16, int& clipped) {
    return pio_round<BITS>((double)x * (double)((int64_t)1 << (BITS - 1)) + (double)d16 * (1.0 / 65536.0), clipped);
}

template <int FMT> struct PioEnc;
template <> struct PioEnc<SOS_ENC_S16> {
    typedef int16_t T;
    static __device__ __forceinline__ T put(float x, int& n) { return (T)pio_quantise<16>(x, n); }
    static __device__ __forceinline__ T put(float x, int32_t d16, int& n) { return (T)pio_quantise<16>(x, d16, n); }
};
template <> struct PioEnc<SOS_ENC_S32> { typedef int32_t T; static __device__ __forceinline__ T put(float x, int& n) { return (T)pio_quantise<32>(x, n); } };
template <> struct PioEnc<SOS_ENC_U8> {
    typedef uint8_t T;
    static __device__ __forceinline__ T put(float x, int& n) { return (T)(pio_quantise<8>(x, n) + 128); }
    static __device__ __forceinline__ T put(float x, int32_t d16, int& n) { return (T)(pio_quantise<8>(x, d16, n) + 128); }
};
template <> struct PioEnc<SOS_ENC_F32> { typedef float T; static __device__ __forceinline__ T put(float x, int&) { return x; } };
// G.711: the s16 value (counted as 's16' counts), then the compressor of pcm_core.h.  The laws' WAVE tags 6 / 7 continue SOS_ENC_*.
template <> struct PioEnc<SOS_G711_ALAW> { typedef G711A T; static __device__ __forceinline__ T put(float x, int& n) { return T{g711_alaw_compress(pio_quantise<16>(x, n))}; } };
template <> struct PioEnc<SOS_G711_ULAW> { typedef G711U T; static __device__ __forceinline__ T put(float x, int& n) { return T{g711_ulaw_compress(pio_quantise<16>(x, n))}; } };

// element e of a file's interleaved output: plane[c][i], 0 from the plane's end on
struct PioPlanes {
    const float* p;
    int64_t avail, ch;
    __device__ __forceinline__ float at(int64_t i, int64_t c) const { return i < avail ? p[c * avail + i] : 0.f; }
};

// the file's count: the workgroup's waves add up in LDS, then one integer atomic per workgroup that counted anything (integer
// adds commute: the same sum on every run).  Every thread of the workgroup calls it.
__device__ __forceinline__ void pio_add_clipped(int clipped, int64_t* dst) {
    __shared__ int block_count;
    if (threadIdx.x == 0) block_count = 0;
    __syncthreads();
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) clipped += __shfl_down(clipped, s, 64);
    if ((threadIdx.x & 63) == 0 && clipped) atomicAdd(&block_count, clipped);
    __syncthreads();
    if (threadIdx.x == 0 && block_count) atomicAdd((unsigned long long*)dst, (unsigned long long)block_count);
}

// KIND: 0, or SOS_DITHER_*.  The seed is an argument of the dithered instantiations only (Seed = uint64_t once, or nothing), so
// that kind 0 keeps the argument list, and with it every instruction, of the kernel before there was a dither.
template <int FMT, int KIND = 0, typename... Seed>
__global__ __launch_bounds__(PIO_THREADS) void pcm_encode_kernel(const float* __restrict__ planes, const int64_t* __restrict__ table,
                                                                 int64_t total_in, int64_t total_out,
                                                                 typename PioEnc<FMT>::T* __restrict__ out,
                                                                 int64_t* __restrict__ clipped, Seed... seed) {
    typedef typename PioEnc<FMT>::T T;
    const int64_t* te = table + (int64_t)blockIdx.y * (KIND ? PIO_DITHER_COLS : PIO_ENCODE_COLS);
    const int64_t first = te[0], avail = te[1], ch = te[2], frames = te[3], ooff = te[4];
    if (!pio_inside(first, avail, ch, total_in) || !pio_inside(ooff, frames, ch, total_out)) return;
    const int64_t n = frames * ch;
    const PioPlanes pl{planes + first, avail, ch};
    T* dst = out + ooff;
    const bool dst_vec = ((uintptr_t)dst & (4 * sizeof(T) - 1)) == 0;
    const bool src_vec = ch == 1 && ragged_aligned16(pl.p);
    int count = 0;
    for (int64_t e0 = ((int64_t)blockIdx.x * PIO_THREADS + threadIdx.x) * 4; e0 < n; e0 += (int64_t)gridDim.x * PIO_THREADS * 4) {
        const bool full = e0 + 4 <= n;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (ch == 1) {
            const int64_t end = n < avail ? n : avail;           // zeros from the plane's end on
            ragged_load4(pl.p, e0, end, src_vec && e0 + 4 <= end, v);
        } else {
            int64_t i = e0 / ch, c = e0 - i * ch;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e0 + k < n) v[k] = pl.at(i, c);
                if (++c == ch) { c = 0; ++i; }
            }
        }
        PioVec4<T> q;
        if constexpr (KIND == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int hit = 0;
                q.v[k] = PioEnc<FMT>::put(v[k], hit);
                if (e0 + k < n) count += hit;
            }
        } else {
            DitherWords words(seed..., (uint32_t)te[5]);
            const uint64_t frame0 = (uint64_t)te[6];
            uint64_t fi[4];                                      // frame and channel of the four elements
            uint32_t fc[4];
            int64_t i = ch == 1 ? e0 : e0 / ch, c = e0 - i * ch;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                fi[k] = frame0 + (uint64_t)i; fc[k] = (uint32_t)c;
                if (++c == ch) { c = 0; ++i; }
            }
            auto put = [&](int k) __attribute__((always_inline)) {
                int hit = 0;
                q.v[k] = PioEnc<FMT>::put(v[k], words.template lsb16<KIND>(fi[k], fc[k]), hit);
                if (e0 + k < n) count += hit;
            };
            if (ch == 2) { put(0); put(2); put(1); put(3); }     // a channel's two frames one after the other: they share a block
            else { put(0); put(1); put(2); put(3); }
        }
        if (full && dst_vec) {
            *(PioVec4<T>*)(dst + e0) = q;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < n) dst[e0 + k] = q.v[k];
        }
    }
    if (FMT != SOS_ENC_F32) pio_add_clipped(count, clipped + blockIdx.y);
}

// packed s24: thread u of a file owns the twelve bytes [12 u - lead, 12 u - lead + 12) of the file's 3 n bytes, lead = the
// file's first byte address mod 4, i.e. three ALIGNED dwords.  They hold (parts of) at most five samples; a sample is counted
// by the thread that owns its first byte.  Whole dwords where all twelve bytes are the file's, single bytes at its two ends.
// A sample astride two units is quantised by both threads: with a dither both draw the same value, a function of its frame.
template <int KIND = 0, typename... Seed>
__global__ __launch_bounds__(PIO_THREADS) void pcm_encode_s24_kernel(const float* __restrict__ planes, const int64_t* __restrict__ table,
                                                                     int64_t total_in, int64_t total_out, uint8_t* __restrict__ out,
                                                                     int64_t* __restrict__ clipped, Seed... seed) {
    const int64_t* te = table + (int64_t)blockIdx.y * (KIND ? PIO_DITHER_COLS : PIO_ENCODE_COLS);
    const int64_t first = te[0], avail = te[1], ch = te[2], frames = te[3], ooff = te[4];
    if (!pio_inside(first, avail, ch, total_in) || !pio_inside(ooff, frames, ch, total_out)) return;
    const int64_t n = frames * ch, nbytes = 3 * n;
    const PioPlanes pl{planes + first, avail, ch};
    uint8_t* dst = out + 3 * ooff;
    const int64_t lead = (int64_t)((uintptr_t)dst & 3);
    const int64_t units = (nbytes + lead + 11) / 12;
    int count = 0;
    for (int64_t u = (int64_t)blockIdx.x * PIO_THREADS + threadIdx.x; u < units; u += (int64_t)gridDim.x * PIO_THREADS) {
        const int64_t p = 12 * u - lead;                         // first byte of the unit, relative to the file (< 0 only for u = 0)
        const int64_t e_lo = p > 0 ? p / 3 : 0;
        int64_t i = e_lo / ch, c = e_lo - i * ch;
        unsigned __int128 bits = 0;                              // the five samples' bytes, little-endian, back to back
        if constexpr (KIND == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int64_t e = e_lo + k;
                if (e < n && 3 * e < p + 12) {
                    int hit = 0;
                    const int32_t q = pio_quantise<24>(pl.at(i, c), hit);
                    if (3 * e >= p) count += hit;                // its first byte is this unit's
                    bits |= (unsigned __int128)((uint32_t)q & 0xffffffu) << (24 * k);
                }
                if (++c == ch) { c = 0; ++i; }
            }
        } else {
            DitherWords words(seed..., (uint32_t)te[5]);
            const uint64_t frame0 = (uint64_t)te[6];
            int64_t fi[5], fc[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                fi[k] = i; fc[k] = c;
                if (++c == ch) { c = 0; ++i; }
            }
            auto put = [&](int k) __attribute__((always_inline)) {
                const int64_t e = e_lo + k;
                if (e < n && 3 * e < p + 12) {
                    int hit = 0;
                    const int32_t q = pio_quantise<24>(pl.at(fi[k], fc[k]), words.template lsb16<KIND>(frame0 + (uint64_t)fi[k], (uint32_t)fc[k]), hit);
                    if (3 * e >= p) count += hit;
                    bits |= (unsigned __int128)((uint32_t)q & 0xffffffu) << (24 * k);
                }
            };
            if (ch == 2) { put(0); put(2); put(4); put(1); put(3); }    // a channel's frames one after the other, as in pcm_encode_kernel
            else { put(0); put(1); put(2); put(3); put(4); }
        }
        const int64_t shift = p - 3 * e_lo;                      // 0 .. 2, or -lead for the unit that begins before the file
        bits = shift >= 0 ? bits >> (8 * shift) : bits << (-8 * shift);
        const uint32_t w[3] = {(uint32_t)bits, (uint32_t)(bits >> 32), (uint32_t)(bits >> 64)};
        if (p >= 0 && p + 12 <= nbytes) {
            uint32_t* d = (uint32_t*)(dst + p);
            d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
        } else {
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (p + b >= 0 && p + b < nbytes) dst[p + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
        }
    }
    pio_add_clipped(count, clipped + blockIdx.y);
}

// Host: the rows [off_col, + table[len_col] * table[ch_col]) of both sides.  Sums each side, then holds every row to the sums;
// returns nfiles, or the first row it cannot accept (what is wrong goes to `why`).
struct PioSide { int off_col, len_col; int64_t total = 0, longest = 0; };
static int pio_check_rows(const int64_t* table, int nfiles, int cols, int ch_col, PioSide* a, PioSide* b, const char** why) {
    for (int f = 0; f < nfiles; ++f) {
        const int64_t* te = table + (int64_t)f * cols;
        const int64_t ch = te[ch_col];
        if (ch < 1 || ch > PIO_MAX_CHANNELS) { *why = "channels outside 1 .. 64"; return f; }
        for (PioSide* s : {a, b}) {
            const int64_t len = te[s->len_col];
            if (len < 0 || len > (INT64_MAX / 8 - s->total) / ch) { *why = "a length that is negative or too large"; return f; }
            s->total += len * ch;
            s->longest = std::max(s->longest, len * ch);
        }
    }
    for (int f = 0; f < nfiles; ++f) {
        const int64_t* te = table + (int64_t)f * cols;
        for (PioSide* s : {a, b})
            if (!pio_inside(te[s->off_col], te[s->len_col], te[ch_col], s->total)) { *why = "a span outside the totals of the table"; return f; }
    }
    return nfiles;
}

// The host half of the decode entry points (`what` = "sample format" / "law", `known` = the caller knows `code`): refuses, or
// sums the table into `in` and sizes the grid.
static int pio_planes_args(const char* who, const void* pcm, const char* what, bool known, int code, const int64_t* table,
                           const int64_t* table_host, int nfiles, const float* out, PioSide* in, dim3* grid) {
    if (!pcm || !table || !table_host || !out) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (!ragged_clips_ok(table_host, nfiles)) {
        sos_set_error("%s: bad args (1 .. 65535 files, got %d)", who, nfiles);
        return SOS_EINVAL;
    }
    if (!known) {
        sos_set_error("%s: unknown %s %d", who, what, code);
        return SOS_EINVAL;
    }
    PioSide pl{3, 1};
    const char* why = "";
    const int bad = pio_check_rows(table_host, nfiles, PIO_PLANES_COLS, 2, in, &pl, &why);
    if (bad < nfiles) {
        const int64_t* te = table_host + (int64_t)bad * PIO_PLANES_COLS;
        sos_set_error("%s: file %d (pcm element %lld, %lld frames, %lld channels, output %lld) has %s (%lld "
                      "elements)", who, bad, (long long)te[0], (long long)te[1], (long long)te[2], (long long)te[3], why, (long long)in->total);
        return SOS_EINVAL;
    }
    *grid = dim3(ragged_grid((in->longest + 3) / 4, PIO_THREADS, PIO_MAX_GRID), (unsigned)nfiles);
    return SOS_OK;
}

// The same for the encode entry points; clears the counts.
static int pio_encode_args(const char* who, const float* planes, const char* what, bool known, int code, const int64_t* table,
                           const int64_t* table_host, int nfiles, const void* out, int64_t* clipped, hipStream_t st,
                           PioSide* in, PioSide* enc, dim3* grid, int cols = PIO_ENCODE_COLS) {
    if (!planes || !table || !table_host || !out || !clipped) { sos_set_error("%s: null pointer", who); return SOS_EINVAL; }
    if (!ragged_clips_ok(table_host, nfiles)) {
        sos_set_error("%s: bad args (1 .. 65535 files, got %d)", who, nfiles);
        return SOS_EINVAL;
    }
    if (!known) {
        sos_set_error("%s: unknown %s %d", who, what, code);
        return SOS_EINVAL;
    }
    const char* why = "";
    const int bad = pio_check_rows(table_host, nfiles, cols, 2, in, enc, &why);
    if (bad < nfiles) {
        const int64_t* te = table_host + (int64_t)bad * cols;
        sos_set_error("%s: file %d (plane sample %lld, %lld available, %lld channels, %lld frames, output element "
                      "%lld) has %s (%lld plane samples, %lld output elements)", who, bad, (long long)te[0], (long long)te[1],
                      (long long)te[2], (long long)te[3], (long long)te[4], why, (long long)in->total, (long long)enc->total);
        return SOS_EINVAL;
    }
    for (int f = 0; cols == PIO_DITHER_COLS && f < nfiles; ++f) {
        const int64_t* te = table_host + (int64_t)f * cols;
        if (te[5] < 0 || te[5] > (int64_t)UINT32_MAX) {
            sos_set_error("%s: file %d has the dither key %lld outside 0 .. 2^32 - 1", who, f, (long long)te[5]);
            return SOS_EINVAL;
        }
        if (te[6] < 0 || te[6] > DITHER_FRAME_LIMIT - te[3]) {
            sos_set_error("%s: file %d has the first frame %lld outside 0 .. 2^62 - its %lld frames", who, f, (long long)te[6],
                          (long long)te[3]);
            return SOS_EINVAL;
        }
    }
    if (hipMemsetAsync(clipped, 0, (size_t)nfiles * sizeof(int64_t), st) != hipSuccess) {
        sos_set_error("%s: cannot clear the counts", who);
        return SOS_ELAUNCH;
    }
    // s24: a thread per twelve bytes = four elements, plus the unit a file that starts off a dword adds
    *grid = dim3(ragged_grid((enc->longest + 3) / 4 + 1, PIO_THREADS, PIO_MAX_GRID), (unsigned)nfiles);
    return SOS_OK;
}

#define PIO_PLANES_GO(T) hipLaunchKernelGGL(pcm_planes_kernel<T>, grid, dim3(PIO_THREADS), 0, st, (const T*)pcm, table, in.total, out)
#define PIO_ENCODE_GO(F) hipLaunchKernelGGL(pcm_encode_kernel<F>, grid, dim3(PIO_THREADS), 0, st, planes, table, in.total, enc.total, \
                                            (PioEnc<F>::T*)out, clipped)

extern "C" int sos_pcm_planes_batch_f32(const void* pcm, int format, const int64_t* table, const int64_t* table_host, int nfiles,
                                        float* out, sos_stream_t stream) {
    const bool known = format == SOS_PCM_S16 || format == SOS_PCM_S32 || format == SOS_PCM_F32 || format == SOS_PCM_U8;
    PioSide in{0, 1};
    dim3 grid;
    const int rc = pio_planes_args("sos_pcm_planes_batch_f32", pcm, "sample format", known, format, table, table_host, nfiles, out, &in, &grid);
    if (rc != SOS_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (format) {
    case SOS_PCM_S16: PIO_PLANES_GO(int16_t); break;
    case SOS_PCM_S32: PIO_PLANES_GO(int32_t); break;
    case SOS_PCM_U8: PIO_PLANES_GO(uint8_t); break;
    default: PIO_PLANES_GO(float); break;
    }
    return sos_check_launch("sos_pcm_planes_batch_f32");
}

extern "C" int sos_g711_planes_batch_f32(const void* codes, int law, const int64_t* table, const int64_t* table_host, int nfiles,
                                         float* out, sos_stream_t stream) {
    const void* pcm = codes;                                     // PIO_PLANES_GO's name for the interleaved side
    PioSide in{0, 1};
    dim3 grid;
    const int rc = pio_planes_args("sos_g711_planes_batch_f32", pcm, "law", law == SOS_G711_ALAW || law == SOS_G711_ULAW, law, table,
                                   table_host, nfiles, out, &in, &grid);
    if (rc != SOS_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (law == SOS_G711_ALAW) PIO_PLANES_GO(G711A); else PIO_PLANES_GO(G711U);
    return sos_check_launch("sos_g711_planes_batch_f32");
}

extern "C" int sos_pcm_encode_batch(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles, int format,
                                    void* out, int64_t* clipped, sos_stream_t stream) {
    const bool known = format == SOS_ENC_S16 || format == SOS_ENC_S24 || format == SOS_ENC_S32 || format == SOS_ENC_U8 || format == SOS_ENC_F32;
    PioSide in{0, 1}, enc{4, 3};
    dim3 grid;
    hipStream_t st = (hipStream_t)stream;
    const int rc = pio_encode_args("sos_pcm_encode_batch", planes, "sample format", known, format, table, table_host, nfiles, out, clipped,
                                   st, &in, &enc, &grid);
    if (rc != SOS_OK) return rc;
    switch (format) {
    case SOS_ENC_S16: PIO_ENCODE_GO(SOS_ENC_S16); break;
    case SOS_ENC_S32: PIO_ENCODE_GO(SOS_ENC_S32); break;
    case SOS_ENC_U8: PIO_ENCODE_GO(SOS_ENC_U8); break;
    case SOS_ENC_F32: PIO_ENCODE_GO(SOS_ENC_F32); break;
    default: hipLaunchKernelGGL(pcm_encode_s24_kernel<>, grid, dim3(PIO_THREADS), 0, st, planes, table, in.total, enc.total,
                                (uint8_t*)out, clipped); break;
    }
    return sos_check_launch("sos_pcm_encode_batch");
}

extern "C" int sos_g711_encode_batch(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles, int law,
                                     void* out, int64_t* clipped, sos_stream_t stream) {
    PioSide in{0, 1}, enc{4, 3};
    dim3 grid;
    hipStream_t st = (hipStream_t)stream;
    const int rc = pio_encode_args("sos_g711_encode_batch", planes, "law", law == SOS_G711_ALAW || law == SOS_G711_ULAW, law, table,
                                   table_host, nfiles, out, clipped, st, &in, &enc, &grid);
    if (rc != SOS_OK) return rc;
    if (law == SOS_G711_ALAW) PIO_ENCODE_GO(SOS_G711_ALAW); else PIO_ENCODE_GO(SOS_G711_ULAW);
    return sos_check_launch("sos_g711_encode_batch");
}

// The dithered encode: the rows, checks and grid of sos_pcm_encode_batch, two more columns per row.
#define PIO_DITHER_GO(F, K) hipLaunchKernelGGL((pcm_encode_kernel<F, K, uint64_t>), grid, dim3(PIO_THREADS), 0, st, planes, table, in.total, \
                                               enc.total, (PioEnc<F>::T*)out, clipped, seed)
#define PIO_DITHER_S24_GO(K) hipLaunchKernelGGL((pcm_encode_s24_kernel<K, uint64_t>), grid, dim3(PIO_THREADS), 0, st, planes, table, in.total, \
                                                enc.total, (uint8_t*)out, clipped, seed)
extern "C" int sos_pcm_encode_dither_batch(const float* planes, const int64_t* table, const int64_t* table_host, int nfiles, int format,
                                           int dither, uint64_t seed, void* out, int64_t* clipped, sos_stream_t stream) {
    const char* who = "sos_pcm_encode_dither_batch";
    if (dither != SOS_DITHER_TPDF && dither != SOS_DITHER_HIGHPASS) {
        sos_set_error("%s: unknown dither %d (SOS_DITHER_TPDF = 1, SOS_DITHER_HIGHPASS = 2)", who, dither);
        return SOS_EINVAL;
    }
    if (format == SOS_ENC_S32 || format == SOS_ENC_F32 || format == SOS_G711_ALAW || format == SOS_G711_ULAW) {
        sos_set_error("%s: sample format %d takes no dither (S16, S24 and U8 do: S32 holds more bits than a float, F32 is a copy, "
                      "G.711 drops the low bits)", who, format);
        return SOS_EINVAL;
    }
    const bool known = format == SOS_ENC_S16 || format == SOS_ENC_S24 || format == SOS_ENC_U8;
    PioSide in{0, 1}, enc{4, 3};
    dim3 grid;
    hipStream_t st = (hipStream_t)stream;
    const int rc = pio_encode_args(who, planes, "sample format", known, format, table, table_host, nfiles, out, clipped, st, &in, &enc,
                                   &grid, PIO_DITHER_COLS);
    if (rc != SOS_OK) return rc;
    const bool tpdf = dither == SOS_DITHER_TPDF;
    switch (format) {
    case SOS_ENC_S16: if (tpdf) PIO_DITHER_GO(SOS_ENC_S16, SOS_DITHER_TPDF); else PIO_DITHER_GO(SOS_ENC_S16, SOS_DITHER_HIGHPASS); break;
    case SOS_ENC_U8: if (tpdf) PIO_DITHER_GO(SOS_ENC_U8, SOS_DITHER_TPDF); else PIO_DITHER_GO(SOS_ENC_U8, SOS_DITHER_HIGHPASS); break;
    default: if (tpdf) PIO_DITHER_S24_GO(SOS_DITHER_TPDF); else PIO_DITHER_S24_GO(SOS_DITHER_HIGHPASS); break;
    }
    return sos_check_launch(who);
}
#undef PIO_DITHER_GO
#undef PIO_DITHER_S24_GO
#undef PIO_PLANES_GO
#undef PIO_ENCODE_GO
