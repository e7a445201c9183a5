"""ITU-R BS.1770-4 / EBU R128 integrated loudness and the gain to a target, stated once in float64 (numpy; scipy.signal.lfilter
where it imports, a plain loop otherwise).  Test infrastructure like the other *_reference.py files: what csrc/loudness.hip,
metrics.loudness_batch and audio_io.loudness_gain_batch_device are held against, never the code under test.
tests/test_loudness_reference.py holds it against the standard's 48 kHz coefficient table and the EBU Tech 3341 signals."""
import math

import numpy as np

try:
    from scipy.signal import lfilter as _lfilter
except ImportError:                                      # pragma: no cover
    _lfilter = None

# ITU-R BS.1770-4, table 1 and table 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, then of the high-pass
TABLE_48K = np.asarray([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                        1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621], dtype=np.float64)


def k_weighting(sr):
    """float64 [10] = {b0, b1, b2, a1, a2} of the shelf and of the high-pass at `sr` Hz (libebur128's closed forms)."""
    sr = float(sr)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    out = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
           2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    return np.asarray(out + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)


def biquad(b, a, x):
    """x through one biquad, transposed direct form II, zero initial state (what lfilter computes)."""
    if _lfilter is not None:
        return _lfilter(b, a, x)
    y, s1, s2 = np.empty_like(x), 0.0, 0.0
    for i, v in enumerate(x):
        o = b[0] * v + s1
        s1 = b[1] * v - a[1] * o + s2
        s2 = b[2] * v - a[2] * o
        y[i] = o
    return y


def weighted(x, sr):
    """One channel plane through both stages, float64."""
    k = k_weighting(sr)
    x = np.asarray(x, dtype=np.float64)
    return biquad(k[5:8], np.r_[1.0, k[8:10]], biquad(k[0:3], np.r_[1.0, k[3:5]], x))


def hop(sr):
    return (int(sr) + 5) // 10


def extent(planes, frames=None):
    """The (channels, frames) samples the encode reads: the plane cropped, or zero-filled past its end."""
    planes = np.asarray(planes)
    planes = planes.reshape(1, -1) if planes.ndim == 1 else planes
    frames = planes.shape[1] if frames is None else int(frames)
    out = np.zeros((planes.shape[0], frames), dtype=planes.dtype)
    n = min(frames, planes.shape[1])
    out[:, :n] = planes[:, :n]
    return out


def block_energies(planes, sr, weights=None, frames=None):
    """z[j] of every whole 400 ms block (one every 100 ms) and l[j] = -0.691 + 10 log10 z[j]."""
    x = extent(planes, frames)
    w = np.ones(x.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    assert w.shape == (x.shape[0],)
    h, n = hop(sr), x.shape[1]
    J = (n - 4 * h) // h + 1 if n >= 4 * h else 0
    z = np.zeros(J, dtype=np.float64)
    for c in range(x.shape[0]):
        if J:                                            # a block is four consecutive hops: its mean square from their sums
            hops = (weighted(x[c], sr)[:(J + 3) * h] ** 2).reshape(J + 3, h).sum(axis=1)
            z += w[c] * (hops[0:J] + hops[1:J + 1] + hops[2:J + 2] + hops[3:J + 3]) / (4.0 * h)
    with np.errstate(divide="ignore"):
        return z, -0.691 + 10.0 * np.log10(z)


def measure(planes, sr, weights=None, frames=None):
    """dict(lufs, peak, blocks, blocks_abs, margin): the integrated loudness, the sample peak max |x| over the extent, the two
    block counts, and the smallest distance in LU of any block from either of its gates."""
    x = extent(planes, frames)
    z, l = block_energies(planes, sr, weights, frames)
    peak = float(np.max(np.abs(x))) if x.size else 0.0
    keep = l > -70.0
    margin = float(np.min(np.abs(l + 70.0))) if l.size else np.inf
    if not keep.any():
        return dict(lufs=-np.inf, peak=peak, blocks=0, blocks_abs=0, margin=margin)
    gate = -0.691 + 10.0 * np.log10(np.mean(z[keep])) - 10.0
    both = keep & (l > gate)
    margin = min(margin, float(np.min(np.abs(l[keep] - gate))))
    lufs = -0.691 + 10.0 * np.log10(np.mean(z[both])) if both.any() else -np.inf
    return dict(lufs=float(lufs), peak=peak, blocks=int(both.sum()), blocks_abs=int(keep.sum()), margin=margin)


def gain(lufs, peak, target, ceiling_db=-1.0):
    """(g as float32, limited): g = min(10^((T - L) / 20), 10^(P / 20) / peak) in float64; 1 where L, T or the peak give none."""
    if not (np.isfinite(lufs) and np.isfinite(target) and peak > 0):
        return np.float32(1.0), False
    to_target, to_ceiling = 10.0 ** ((target - lufs) / 20.0), 10.0 ** (ceiling_db / 20.0) / peak
    return np.float32(min(to_target, to_ceiling)), bool(to_ceiling < to_target)


def apply_gain(planes, g, frames=None):
    """planes (float32) with the first `frames` samples of every channel times g, one float32 multiply each."""
    out = np.array(planes, dtype=np.float32, copy=True)
    n = out.shape[1] if frames is None else min(int(frames), out.shape[1])
    out[:, :n] = out[:, :n] * np.float32(g)
    return out


def sine(freq, sr, segments, channels=1):
    """A sine whose peak level steps through `segments` = [(dBFS, seconds), ..], the same in every channel: float32 (channels, n)."""
    amp = np.concatenate([np.full(int(round(sec * sr)), 10.0 ** (db / 20.0)) for db, sec in segments])
    x = (amp * np.sin(2.0 * np.pi * freq * np.arange(amp.size) / sr)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(x, (channels, x.size)))


# EBU Tech 3341 (2016), table 1, cases 1-5: stereo 1 kHz sine in phase, peak levels in dBFS -> the reading in LUFS (+-0.1)
TECH_3341 = {
    1: ([(-23.0, 20.0)], -23.0),
    2: ([(-33.0, 20.0)], -33.0),
    3: ([(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)], -23.0),
    4: ([(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)], -23.0),
    5: ([(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)], -23.0),
}
