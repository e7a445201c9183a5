// pcm_core.h -- the one statement of the sample-to-float rule (wave_io.hip's mono decode, pcm_io.hip's channel planes):
// soundfile's decode, integer PCM / 2^(bits-1); u8 is offset binary; f32 passes through.  24-bit PCM is carried in the top
// three bytes of an int32 (audio_io.read_wave).
#pragma once
#include "sos_common.h"

template <typename T> struct Pcm;
template <> struct Pcm<int16_t> { static __device__ __forceinline__ float cvt(int16_t v) { return (float)v * (1.0f / 32768.0f); } };
template <> struct Pcm<int32_t> { static __device__ __forceinline__ float cvt(int32_t v) { return (float)((double)v * (1.0 / 2147483648.0)); } };
template <> struct Pcm<uint8_t> { static __device__ __forceinline__ float cvt(uint8_t v) { return ((float)v - 128.0f) * (1.0f / 128.0f); } };
template <> struct Pcm<float> { static __device__ __forceinline__ float cvt(float v) { return v; } };
