// dither_core.h -- the one statement of the dither the encode kernels of pcm_io.hip add before they round (u8 / s16 / s24;
// include/sos_hip.h: sos_pcm_encode_dither_batch; numpy restatement: tests/dither_reference.py).  The dither of a sample is a
// pure function of (seed, file key, channel, absolute frame): no state, no pass of its own over the planes, so a file's bytes
// do not depend on the other files of its launch, on the grid, on the access path, or on how a live leg was cut into packets,
// and the two threads of the packed-s24 kernel that both quantise a sample astride their units draw the same value.
//
// Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123).
//   round: c' = {hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0)}, M0 = 0xD2511F53, M1 = 0xCD9E8D57;
//   ten rounds, the key bumped by {0x9E3779B9, 0xBB67AE85} after every round.  Random123's known answers:
//   counter {0,0,0,0}, key {0,0} -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; all ffffffff -> 408f276d 41c83b0e a20bc7c6 6d5451fd.
// Word of a sample: n = frame0 + i, the absolute frame (0 <= n < 2^62).  Counter {low32(n >> 2), high32(n >> 2), channel, file
//   key}, key {low32(seed), high32(seed)}; w(n) = output word n & 3 of that block: one block serves four consecutive frames of
//   one channel.
// Dither in LSB, an exact integer over 2^16:
//   SOS_DITHER_TPDF      d = ((w & 0xFFFF) - (w >> 16)) / 65536: triangular on (-1, 1), variance 1/6
//   SOS_DITHER_HIGHPASS  d[n] = (u(n + 1) - u(n)) / 65536, u(n) = w(n) & 0xFFFF: the same marginal, spectrum (1/12)(2 - 2 cos w),
//                        moved towards fs/2.  It shapes the DITHER only: the quantisation error is not fed back.
// Quantiser: q = rint((double)x * S + d) half to even, then pio_quantise's rule (NaN -> 0, saturated to [-S, S - 1], counted
//   AFTER the dither).  x * S is exact in double (a float times a power of two), so fma(x, S, d) and multiply-then-add round the
//   same exact sum once: the compiler's contraction (-ffp-contract=on) cannot change a byte.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define DITHER_FRAME_LIMIT ((int64_t)1 << 62)      // frame0 + frames may not pass it

__host__ __device__ static inline uint32_t dither_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// c = Philox4x32-10(counter c, key k), in place.  Scalars, not arrays, here and in DitherWords, and word n & 3 picked by selects
// on its two bits: an array indexed by n & 3 (and a chain of comparisons with 0 .. 3, which the compiler turns into one) is placed
// in scratch memory; four registers under three selects are not.
__host__ __device__ static inline __attribute__((always_inline)) void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3,
                                                                                    uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = dither_mulhi(M0, c0), l0 = M0 * c0, h1 = dither_mulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// The words of one file for one thread.  It keeps the last block: asked for frames in rising order within a channel, it runs
// Philox once per (channel, n >> 2) -- one or two blocks for four consecutive frames, at most one more for 'highpass'.
struct DitherWords {
    uint32_t k0, k1, file_key;
    uint64_t have_block = ~(uint64_t)0;              // no n >> 2 reaches it
    uint32_t have_channel = 0;
    uint32_t w0, w1, w2, w3;
    __host__ __device__ DitherWords(uint64_t seed, uint32_t key) : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)), file_key(key) {}

    __host__ __device__ inline uint32_t word(uint64_t n, uint32_t channel) {
        const uint64_t block = n >> 2;
        if (block != have_block || channel != have_channel) {
            w0 = (uint32_t)block; w1 = (uint32_t)(block >> 32); w2 = channel; w3 = file_key;
            philox4x32_10(w0, w1, w2, w3, k0, k1);
            have_block = block; have_channel = channel;
        }
        const uint32_t lo = n & 1 ? w1 : w0, hi = n & 1 ? w3 : w2;
        return n & 2 ? hi : lo;
    }

    // 65536 d of frame n: an integer in (-65536, 65536).  KIND: SOS_DITHER_TPDF = 1, SOS_DITHER_HIGHPASS = 2
    template <int KIND> __host__ __device__ inline int32_t lsb16(uint64_t n, uint32_t channel) {
        if (KIND == 1) {
            const uint32_t v = word(n, channel);
            return (int32_t)(v & 0xFFFF) - (int32_t)(v >> 16);
        }
        const int32_t u0 = (int32_t)(word(n, channel) & 0xFFFF);
        return (int32_t)(word(n + 1, channel) & 0xFFFF) - u0;
    }
};
