"""The look-ahead limiter of csrc/limiter.hip / audio_io.limit_batch_device, stated once in numpy on top of
tests/loudness_reference.py and tests/r128_reference.py.  Test infrastructure like the other *_reference.py files: what the kernel
is held against, never the code under test.  tests/test_limiter_reference.py holds it to the properties the rule is built for.
The rule is the project's own -- symmetric, parallel, no recurrence -- and ONE gain curve serves all channels of a file.  With m =
min(frames, available) and samples outside [0, m) reading 0:
  s     = float32(10^((T - L) / 20)) from float64, 1 where L or T is not finite;  C = float32(10^(P / 20))
  p[t]  = max over channels of |x[t]| ('sample'); under 'true' also of the six interpolated points next to t, t - 1 + q / 4 and
          t + q / 4 for q = 1, 2, 3 (r128_reference.interpolated: float64 sums of the float32 products, rounded to float32 once;
          the kernel sums with 12 fmaf in float32, which is where the two may differ)
  a     = s * p[t], one float32 multiply;  r[t] = a > C ? max(float32(float64(C) / float64(a)), 2^-10) : 1;  r = 1 outside [0, m)
  H     = round(lookahead_ms * rate / 1000), 1 <= H <= 1024
  mn[t] = min r[t - H .. t + H]
  g[t]  = float32((sum of float64(mn[t - H .. t + H])) / (2 H + 1))
  y[t]  = x[t] * (g[t] * s): g * s rounded to float32 first, then one float32 multiply; samples [m, available) are copied
t lies inside the window of every mn[u] that g[t] averages, so g[t] <= r[t]; g ramps linearly over 2 H samples on either side of a
peak.  The floor 2^-10 makes every mn a multiple of 2^-33 (a float32 in [2^-10, 1] has its last bit at 2^-33 or above), and a sum
of at most 2^13 of them needs 46 bits: the float64 sums are EXACT in any order."""
import numpy as np

import loudness_reference as LR
import r128_reference as R

FLOOR = np.float32(2.0 ** -10)
MAX_H = 1024


def lookahead(lookahead_ms, rate):
    """H in samples."""
    return int(round(float(lookahead_ms) * rate / 1000.0))


def to_target(lufs, target):
    """s as float32."""
    if not (np.isfinite(lufs) and np.isfinite(target)):
        return np.float32(1.0)
    return np.float32(10.0 ** ((float(target) - float(lufs)) / 20.0))


def ceiling(ceiling_db):
    """C as float32."""
    return np.float32(10.0 ** (float(ceiling_db) / 20.0))


def envelope(planes, frames=None, true_peak=False):
    """p as float32 [frames] over the extent the encode reads."""
    x = LR.extent(np.asarray(planes, dtype=np.float32), frames)
    if not x.shape[1]:
        return np.zeros(0, dtype=np.float32)
    p = np.max(np.abs(x), axis=0)
    if true_peak:
        q = np.max(np.abs(R.interpolated(x)), axis=(0, 2)).astype(np.float32)      # q[i]: the points (i - 1) + 1/4 .. 3/4
        p = np.maximum(p, np.maximum(q[:-1], q[1:]))
    return p


def reduction(p, s, C, m=None):
    """r as float32: what brings s * p[t] to the ceiling, never below 2^-10; 1 from sample m on."""
    p = np.asarray(p, dtype=np.float32)
    a = p * np.float32(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        down = np.maximum((np.float64(np.float32(C)) / a.astype(np.float64)).astype(np.float32), FLOOR)
    r = np.where(a > np.float32(C), down, np.float32(1.0)).astype(np.float32)
    if m is not None:
        r[m:] = 1.0
    return r


def sliding_min(r, H):
    """mn[u] = min r[u - H .. u + H] for u = -H .. n + H - 1 (every mn the windows of g[0 .. n) read), r = 1 outside [0, n):
    float32 [n + 2 H], by 2 H plain minima."""
    n = r.size
    pad = np.concatenate([np.ones(2 * H, np.float32), np.asarray(r, dtype=np.float32), np.ones(2 * H, np.float32)])
    out = pad[:n + 2 * H].copy()
    for k in range(1, 2 * H + 1):
        np.minimum(out, pad[k:k + n + 2 * H], out=out)
    return out


def window_mean(mn, H):
    """g[t] = float32((mn[t - H] + .. + mn[t + H]) / (2 H + 1)) for t = 0 .. n - 1 from sliding_min's mn, by float64 prefix sums:
    exact while the whole sum stays below 2^20 (53 bits - 33)."""
    n = mn.size - 2 * H
    assert mn.size < 1 << 20
    c = np.concatenate([[0.0], np.cumsum(mn.astype(np.float64))])
    return ((c[2 * H + 1:2 * H + 1 + n] - c[:n]) / np.float64(2 * H + 1)).astype(np.float32)


def gain_curve(p, s, C, H):
    """(g, r), float32 [len(p)] each."""
    assert 1 <= H <= MAX_H
    r = reduction(p, s, C)
    return window_mean(sliding_min(r, H), H), r


def limit(planes, s, ceiling_db, H, frames=None, true_peak=False):
    """dict(y, g, r, p, min_g, samples): the limited planes (float32, the shape of `planes`; samples from min(frames, available) on
    are copied), the curves over [0, m), and what the kernel's row reports: the least g (1 without one below 1) and the number of
    samples with g < 1."""
    x = np.asarray(planes, dtype=np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    m = x.shape[1] if frames is None else min(int(frames), x.shape[1])
    s, C = np.float32(s), ceiling(ceiling_db)
    p = envelope(x[:, :m], None, true_peak)
    g, r = gain_curve(p, s, C, H)
    y = x.copy()
    y[:, :m] = x[:, :m] * (g * s)[None, :]
    below = g < np.float32(1.0)
    return dict(y=y, g=g, r=r, p=p, min_g=float(np.min(g[below])) if below.any() else 1.0, samples=int(below.sum()))
