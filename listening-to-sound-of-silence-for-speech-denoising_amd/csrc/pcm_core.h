// pcm_core.h -- the one statement of the sample-to-float rule (wave_io.hip's mono decode, pcm_io.hip's channel planes):
// soundfile's decode, integer PCM / 2^(bits-1); u8 is offset binary; f32 passes through.  24-bit PCM is carried in the top
// three bytes of an int32 (audio_io.read_wave).  G.711 code bytes (WAVE tags 6 / 7) expand to a linear level / 2^15, and
// compress from the s16 value of a float (pcm_io.hip's pio_quantise<16>): the rule is below, in integers, without a table.
#pragma once
#include "sos_common.h"

template <typename T> struct Pcm;
template <> struct Pcm<int16_t> { static __device__ __forceinline__ float cvt(int16_t v) { return (float)v * (1.0f / 32768.0f); } };
template <> struct Pcm<int32_t> { static __device__ __forceinline__ float cvt(int32_t v) { return (float)((double)v * (1.0 / 2147483648.0)); } };
template <> struct Pcm<uint8_t> { static __device__ __forceinline__ float cvt(uint8_t v) { return ((float)v - 128.0f) * (1.0f / 128.0f); } };
template <> struct Pcm<float> { static __device__ __forceinline__ float cvt(float v) { return v; } };

// ---- G.711 (ITU-T G.711; the arithmetic of the Sun / ITU reference g711.c, which CPython's audioop, libsndfile and sox share).
// A code byte is sign, 3-bit segment, 4-bit step.  One-byte wrappers, so that Pcm<uint8_t> stays the u8 rule and four
// interleaved codes are one dword.
struct G711A { uint8_t c; };
struct G711U { uint8_t c; };

// code -> linear level in s16 units: mu-law within +-32124 (0x7F and 0xFF both give 0), A-law within +-32256
__device__ __forceinline__ int32_t g711_ulaw_expand(uint32_t c) {
    const uint32_t u = ~c & 0xFF;
    const int32_t t = (int32_t)((((u & 15) << 3) + 0x84) << ((u >> 4) & 7));
    return (u & 0x80) ? 0x84 - t : t - 0x84;
}
__device__ __forceinline__ int32_t g711_alaw_expand(uint32_t c) {
    const uint32_t a = (c ^ 0x55) & 0xFF, seg = (a >> 4) & 7;
    const uint32_t t = ((a & 15) << 4) + (seg ? 0x108 : 8);      // segment 0 has no leading one
    const int32_t m = (int32_t)(t << (seg ? seg - 1 : 0));
    return (a & 0x80) ? m : -m;
}

// s16 value -> code: the reference compressor, which drops the low bits (it does not round to the nearest level).  The
// segment is the position of the magnitude's leading one, from a count of leading zeros.
__device__ __forceinline__ uint8_t g711_ulaw_compress(int32_t q) {
    int32_t p = q >> 2;                                          // 14 bits
    const uint32_t mask = p < 0 ? 0x7F : 0xFF;
    p = min(abs(p) + 0x21, 0x1FFF);                              // biased; past the last segment's end is its last step
    const int seg = 26 - __clz(p);                               // p >= 0x21: ends 0x3F, 0x7F, .. 0x1FFF -> 0 .. 7
    return (uint8_t)((((uint32_t)seg << 4) | (((uint32_t)p >> (seg + 1)) & 15)) ^ mask);
}
__device__ __forceinline__ uint8_t g711_alaw_compress(int32_t q) {
    int32_t p = q >> 3;                                          // 13 bits
    const uint32_t mask = p < 0 ? 0x55 : 0xD5;
    p = p < 0 ? -p - 1 : p;                                      // 0 .. 4095
    const int seg = max(27 - __clz(p), 0);                       // ends 0x1F, 0x3F, .. 0xFFF -> 0 .. 7 (__clz(0) = 32)
    return (uint8_t)((((uint32_t)seg << 4) | (((uint32_t)p >> max(seg, 1)) & 15)) ^ mask);
}

template <> struct Pcm<G711A> { static __device__ __forceinline__ float cvt(G711A v) { return (float)g711_alaw_expand(v.c) * (1.0f / 32768.0f); } };
template <> struct Pcm<G711U> { static __device__ __forceinline__ float cvt(G711U v) { return (float)g711_ulaw_expand(v.c) * (1.0f / 32768.0f); } };
