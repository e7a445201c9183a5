"""Numpy restatement of the G.711 sample rule of csrc/pcm_core.h (include/sos_hip.h states it) and of the RIFF/WAVE container
audio_io.wave_container writes around A-law / mu-law data.  Test infrastructure like the oracle: the reference, not the code under
test.  Written from the segment tables of ITU-T G.711 (a code byte = sign, 3-bit segment, 4-bit step within the segment), in
whole numbers throughout, so every level, byte and count below is exact and the tests ask the kernels for equality.
tests/test_g711_reference.py holds it against CPython's audioop (the Sun / ITU g711.c) on all 256 codes and all 65 536 s16 values.

Laws: 'alaw' (WAVE format tag 6), 'ulaw' (tag 7); 8 bits per sample.  The float -> s16 step of the encode is pcm_reference's."""
import struct

import numpy as np

import pcm_reference as P

TAG = {"alaw": 6, "ulaw": 7}
SILENCE = {"alaw": 0xD5, "ulaw": 0xFF}                           # the code of linear 0
PEAK = {"alaw": 32256, "ulaw": 32124}                            # the largest decoded level, in s16 units
# the last magnitude of each of the eight segments: 13-bit A-law, 14-bit biased mu-law
ENDS = {"alaw": np.asarray([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF]),
        "ulaw": np.asarray([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF])}
ULAW_BIAS = 33                                                   # 14-bit units


def expand(codes, law):
    """uint8 codes (any shape) -> int64 linear levels in s16 units (|level| <= PEAK[law])."""
    c = np.asarray(codes).astype(np.int64) & 0xFF
    if law == "ulaw":                                            # stored inverted; sign bit set = negative
        u = c ^ 0xFF
        seg, step = (u >> 4) & 7, u & 15
        mag = 4 * (((2 * step + ULAW_BIAS) << seg) - ULAW_BIAS)  # 14-bit level, times 4
        return np.where(u & 0x80, -mag, mag)
    if law == "alaw":                                            # even bits inverted; sign bit set = positive
        a = c ^ 0x55
        seg, step = (a >> 4) & 7, a & 15
        mag = 8 * np.where(seg == 0, 2 * step + 1, (2 * step + 33) << np.maximum(seg - 1, 0))   # 13-bit level (mid-step), times 8
        return np.where(a & 0x80, mag, -mag)
    raise ValueError(law)


def compress(q, law):
    """int s16 values (any shape) -> uint8 codes: the reference compressor, which drops the low bits (it does not round to the
    nearest level)."""
    q = np.asarray(q).astype(np.int64)
    ends = ENDS[law]
    if law == "ulaw":
        p = q >> 2                                               # 14 bits, floor
        mask = np.where(p < 0, 0x7F, 0xFF)
        mag = np.abs(p) + ULAW_BIAS
        seg = np.searchsorted(ends, mag, side="left")            # the number of segment ends below mag
        code = np.where(seg >= 8, 0x7F, (np.minimum(seg, 7) << 4) | ((mag >> (np.minimum(seg, 7) + 1)) & 15))
        return (code ^ mask).astype(np.uint8)
    if law == "alaw":
        p = q >> 3                                               # 13 bits, floor
        mask = np.where(p < 0, 0x55, 0xD5)
        mag = np.where(p < 0, -p - 1, p)
        seg = np.searchsorted(ends, mag, side="left")
        assert seg.max(initial=0) < 8
        code = (seg << 4) | ((mag >> np.maximum(seg, 1)) & 15)
        return (code ^ mask).astype(np.uint8)
    raise ValueError(law)


def decode(codes, law):
    """(frames, channels) uint8 codes -> (channels, frames) float32 planes: level / 32768 (exact)."""
    return np.ascontiguousarray((expand(codes, law).astype(np.float64) / 32768.0).astype(np.float32).T)


def mono(codes, law):
    """(frames, channels) codes -> (frames,) float32, the expression of the mono kernel: the f32 sum over the channels in order,
    starting from +0.0, times the f32 reciprocal of the channel count (one channel: the sum itself)."""
    planes = decode(codes, law)
    s = np.zeros(planes.shape[1], dtype=np.float32)
    for c in range(planes.shape[0]):
        s = (s + planes[c]).astype(np.float32)
    return s if planes.shape[0] == 1 else (s * (np.float32(1.0) / np.float32(planes.shape[0]))).astype(np.float32)


def encode(planes, law, frames=None):
    """(channels, n) float32 planes -> (bytes of the interleaved [frames][channels] codes, clipped count of the s16 step).  Samples
    past the plane's end are 0, hence SILENCE[law]; frames below n crops."""
    p = np.asarray(planes, dtype=np.float32)
    ch, n = p.shape
    frames = n if frames is None else int(frames)
    x = np.zeros((ch, frames), dtype=np.float32)
    x[:, :min(n, frames)] = p[:, :min(n, frames)]
    q, clipped = P.quantise(np.ascontiguousarray(x.T), "s16")
    return compress(q, law).tobytes(), clipped


def container(data, law, channels, rate):
    """The RIFF/WAVE file around G.711 data: an 18-byte fmt chunk (cbSize 0), a fact chunk with the frame count, the data chunk;
    no pad byte after an odd data chunk."""
    align = channels
    fmt_body = struct.pack("<HHIIHH", TAG[law], channels, rate, rate * align, align, 8) + b"\0\0"
    chunks = b"fmt " + struct.pack("<I", len(fmt_body)) + fmt_body
    chunks += b"fact" + struct.pack("<II", 4, len(data) // align)
    chunks += b"data" + struct.pack("<I", len(data)) + bytes(data)
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks
