"""numpy restatement of the dither of csrc/dither_core.h (include/sos_hip.h: sos_pcm_encode_dither_batch), built on pcm_reference
without touching it.  Test infrastructure like the oracle: the reference, not the code under test.  Everything is integers and
float64 sums of exactly representable terms, so every byte and count is exact and the tests ask the kernels for equality.

Generator: Philox4x32-10 (Salmon et al., Random123).  Word of a sample: n = frame0 + i; counter {low32(n >> 2), high32(n >> 2),
channel, file key}, key {low32(seed), high32(seed)}; w(n) = output word n & 3.  Dither in LSB: 'tpdf' ((w & 0xFFFF) - (w >> 16)) /
65536; 'highpass' (u(n + 1) - u(n)) / 65536 with u = w & 0xFFFF.  q = rint(x * S + d) half to even, NaN -> 0, saturated, counted
after the dither."""
import numpy as np

import pcm_reference as R

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
KINDS = ("tpdf", "highpass")
FORMATS = ("u8", "s16", "s24")


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two -> four uint64 arrays holding the block's 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)          # 32 x 32 bits: fits uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def words(n, channel, seed, key):
    """w(n) of the absolute frames n (int64 array, 0 <= n < 2^62) of one channel of the file with this key."""
    n = np.asarray(n, dtype=np.uint64)
    block = n >> np.uint64(2)
    out = philox4x32_10([block & np.uint64(MASK), block >> np.uint64(32), channel, key], [seed & MASK, (seed >> 32) & MASK])
    j = (n & np.uint64(3)).astype(np.int64)
    return np.choose(j, out)


def dither16(kind, n, channel, seed, key):
    """65536 d for the absolute frames n: int64 in (-65536, 65536)."""
    n = np.asarray(n, dtype=np.int64)
    if kind == "tpdf":
        w = words(n, channel, seed, key).astype(np.int64)
        return (w & 0xFFFF) - (w >> 16)
    if kind == "highpass":
        u0 = words(n, channel, seed, key).astype(np.int64) & 0xFFFF
        u1 = words(n + 1, channel, seed, key).astype(np.int64) & 0xFFFF
        return u1 - u0
    raise ValueError(kind)


def dither_lsb(kind, n, channel, seed, key):
    """d in LSB, float64 (exact)."""
    return dither16(kind, n, channel, seed, key).astype(np.float64) / 65536.0


def quantise(x, fmt, d):
    """float32 array and its dither in LSB (float64, same shape) -> (int64 q, samples that were NaN or changed by saturation)."""
    S = R.scale(fmt)
    t = np.asarray(x, dtype=np.float32).astype(np.float64) * S + d
    nan = np.isnan(t)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.where(nan, 0.0, t))
    hi, lo = r > S - 1.0, r < -S
    q = np.where(hi, S - 1.0, np.where(lo, -S, r)).astype(np.int64)
    return q, int(nan.sum() + hi.sum() + lo.sum())


def encode(planes, fmt, frames=None, dither=None, seed=0, key=0, frame0=0):
    """pcm_reference.encode with the dither: (channels, n) float32 planes -> (bytes of [frames][channels], clipped count).
    dither=None is pcm_reference.encode itself."""
    if dither is None:
        return R.encode(planes, fmt, frames)
    if fmt not in FORMATS:
        raise ValueError(fmt)
    p = np.asarray(planes, dtype=np.float32)
    ch, n = p.shape
    frames = n if frames is None else int(frames)
    x = np.zeros((ch, frames), dtype=np.float32)
    x[:, :min(n, frames)] = p[:, :min(n, frames)]
    at = np.arange(frames, dtype=np.int64) + int(frame0)
    d = np.stack([dither_lsb(dither, at, c, seed, key) for c in range(ch)]) if frames else np.zeros((ch, 0))
    q, clipped = quantise(x, fmt, d)
    q = np.ascontiguousarray(q.T)                              # [frames][channels]
    if fmt == "u8":
        return (q + 128).astype(np.uint8).tobytes(), clipped
    if fmt == "s16":
        return q.astype("<i2").tobytes(), clipped
    u = (q & 0xFFFFFF).reshape(-1)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes(), clipped
