"""Float64 numpy restatement of the channel-plane decode and encode rules of csrc/pcm_io.hip (include/sos_hip.h states them) and
of the RIFF/WAVE container audio_io.wave_container writes.  Test infrastructure like the oracle: the reference, not the code
under test.  A float times a power of two is exact in double, so every byte and every count below is exact, and the tests ask the
kernels for equality.

Formats: 's16', 's24' (3 bytes little-endian, packed), 's32', 'u8' (offset binary), 'f32'."""
import struct

import numpy as np

BITS = {"s16": 16, "s24": 24, "s32": 32, "u8": 8}
WIDTH = {"s16": 2, "s24": 3, "s32": 4, "u8": 1, "f32": 4}
TAG_BITS = {"s16": (1, 16), "s24": (1, 24), "s32": (1, 32), "u8": (1, 8), "f32": (3, 32)}


def scale(fmt):
    return float(2 ** (BITS[fmt] - 1))


def unpack(data, fmt, channels):
    """The bytes of interleaved WAVE data -> integer / float array (frames, channels): int64 for the integer formats (u8 as
    stored, 0 .. 255), float32 for 'f32'."""
    b = np.frombuffer(bytes(data), dtype=np.uint8)
    if fmt == "f32":
        v = b.view("<f4")
    elif fmt == "u8":
        v = b.astype(np.int64)
    elif fmt == "s16":
        v = b.view("<i2").astype(np.int64)
    elif fmt == "s32":
        v = b.view("<i4").astype(np.int64)
    elif fmt == "s24":
        t = b.reshape(-1, 3).astype(np.int64)
        v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        v = v - ((v & 0x800000) << 1)
    else:
        raise ValueError(fmt)
    return v.reshape(-1, channels)


def decode(values, fmt):
    """(frames, channels) samples as unpack gives them -> (channels, frames) float32 planes: sample / 2^(bits-1), u8
    (v - 128) / 128, rounded once to float32; 'f32' as is."""
    v = np.asarray(values)
    if fmt == "f32":
        return np.ascontiguousarray(v.astype(np.float32).T)
    v = v.astype(np.float64)
    if fmt == "u8":
        v = v - 128.0
    return np.ascontiguousarray((v / scale(fmt)).astype(np.float32).T)


def quantise(x, fmt):
    """float32 array -> (int64 q of the same shape, number of samples that were NaN or changed by saturation)."""
    S = scale(fmt)
    d = np.asarray(x, dtype=np.float32).astype(np.float64) * S
    nan = np.isnan(d)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.where(nan, 0.0, d))                   # half to even
    hi, lo = r > S - 1.0, r < -S
    q = np.where(hi, S - 1.0, np.where(lo, -S, r)).astype(np.int64)
    return q, int(nan.sum() + hi.sum() + lo.sum())


def encode(planes, fmt, frames=None):
    """(channels, n) float32 planes -> (bytes of the interleaved [frames][channels] data, clipped count).  Samples past the
    plane's end are 0; frames below n crops."""
    p = np.asarray(planes, dtype=np.float32)
    ch, n = p.shape
    frames = n if frames is None else int(frames)
    x = np.zeros((ch, frames), dtype=np.float32)
    x[:, :min(n, frames)] = p[:, :min(n, frames)]
    x = np.ascontiguousarray(x.T)                            # [frames][channels]
    if fmt == "f32":
        return x.astype("<f4").tobytes(), 0
    q, clipped = quantise(x, fmt)
    if fmt == "u8":
        return (q + 128).astype(np.uint8).tobytes(), clipped
    if fmt == "s16":
        return q.astype("<i2").tobytes(), clipped
    if fmt == "s32":
        return q.astype("<i4").tobytes(), clipped
    u = (q & 0xFFFFFF).reshape(-1)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes(), clipped


def container(data, fmt, channels, rate):
    """The RIFF/WAVE file around encoded data: PCM with a 16-byte fmt chunk; float with an 18-byte fmt chunk (cbSize 0) and a
    fact chunk holding the frame count."""
    tag, bits = TAG_BITS[fmt]
    align = channels * bits // 8
    fmt_body = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits) + (b"" if tag == 1 else b"\0\0")
    chunks = b"fmt " + struct.pack("<I", len(fmt_body)) + fmt_body
    if tag != 1:
        chunks += b"fact" + struct.pack("<II", 4, len(data) // align)
    chunks += b"data" + struct.pack("<I", len(data)) + bytes(data)
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def edge_values(fmt):
    """The inputs whose treatment the rule fixes, as float32: ties, the two ends, beyond them, NaN, infinities, -0.0, denormals."""
    S = scale(fmt) if fmt != "f32" else 32768.0
    return np.asarray([0.5 / S, 1.5 / S, 2.5 / S, -0.5 / S, -1.5 / S, -1.0, 1.0, (S - 1) / S, (S - 0.5) / S, -(S + 0.5) / S, 1.25, -1.25,
                       np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-39, 3e38, -3e38], dtype=np.float32)
