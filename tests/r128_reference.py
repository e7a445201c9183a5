"""The EBU R128 measures beside the integrated loudness, stated once in float64 (numpy) on top of tests/loudness_reference.py: the
TRUE PEAK of a file by the project's own 4x interpolator (ITU-R BS.1770-4 Annex 2 allows any suitable one), the LOUDNESS RANGE
(EBU Tech 3342, libebur128's nearest-rank percentiles) and the maximum momentary / short-term loudness.  Test infrastructure like
the other *_reference.py files: what csrc/loudness.hip's sos_true_peak_batch_f64 / sos_loudness_range_batch_f64 and
metrics.true_peak_batch / loudness_batch(true_peak=, loudness_range=) are held against, never the code under test.
tests/test_r128_reference.py holds it against sines whose true peak and level steps are known in closed form."""
import numpy as np

import loudness_reference as LR

TAPS, HALF, PHASES = 12, 6, 3           # taps per phase k = -5 .. 6, the prototype's half length in samples, phases 1 .. 3 of 4
KAISER_BETA = 9.0


def prototype(u):
    """The interpolator's prototype at `u` samples from its centre: sinc(u) I0(9 sqrt(1 - (u / 6)^2)) / I0(9) inside |u| < 6."""
    u = np.asarray(u, dtype=np.float64)
    inside = np.abs(u) < HALF
    arg = np.sqrt(np.where(inside, 1.0 - (u / HALF) ** 2, 0.0))
    return np.where(inside, np.sinc(u) * np.i0(KAISER_BETA * arg) / np.i0(KAISER_BETA), 0.0)


def true_peak_filter(phase0=False):
    """float64 [3][12]: h_p[k] = prototype(k - p / 4) for p = 1, 2, 3 and k = -5 .. 6; with phase0 a leading row p = 0."""
    k = np.arange(-5, 7, dtype=np.float64)
    return np.stack([prototype(k - p / 4.0) for p in range(0 if phase0 else 1, 4)])


def true_peak_filter_f32():
    """The coefficients every implementation multiplies with: the float64 values rounded to float32 once."""
    return true_peak_filter().astype(np.float32)


def interpolated(planes, frames=None, coef=None):
    """float64 (channels, frames + 1, 3): the values at n + p / 4 for n = -1 .. frames - 1 and p = 1, 2, 3, summed in float64 in
    tap order from the float32 coefficients; samples outside the extent read 0."""
    x = LR.extent(planes, frames).astype(np.float64)
    h = np.asarray(true_peak_filter_f32() if coef is None else coef, dtype=np.float64)
    ch, n = x.shape
    xp = np.zeros((ch, n + TAPS), dtype=np.float64)
    xp[:, HALF:HALF + n] = x                             # x[n + k] of the point n = m - 1 is xp[m + k + 5]
    out = np.zeros((ch, n + 1, PHASES), dtype=np.float64)
    for kk in range(TAPS):
        out += h[None, None, :, kk] * xp[:, kk:kk + n + 1, None]
    return out


def true_peak(planes, frames=None, coef=None):
    """The true peak of a file as a linear value: the maximum of |x| and |v| over all channels, samples and interpolated points."""
    x = LR.extent(planes, frames)
    v = interpolated(planes, frames, coef)
    sample = float(np.max(np.abs(x.astype(np.float64)))) if x.size else 0.0
    return max(sample, float(np.max(np.abs(v))) if v.size else 0.0)


def db(v):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.float64(v))


def faded_sine(period, phase_deg, amp=0.5, n=4096, fade=512):
    """amp sin(2 pi n / period + phase) under a raised-cosine fade in and out: float32 (1, n).  The plateau holds the peaks."""
    t = np.arange(n, dtype=np.float64)
    w = np.ones(n)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(fade) + 0.5) / fade)
    w[:fade], w[n - fade:] = ramp, ramp[::-1]
    return (amp * w * np.sin(2.0 * np.pi * t / period + np.deg2rad(phase_deg))).astype(np.float32).reshape(1, -1)


# ------------------------------------------------------------------------------------------------ loudness range and the maxima
WINDOW_HOPS = 30                        # a short-term window: 3 s = 30 hops, one every hop


def hop_energies(planes, sr, weights=None, frames=None):
    """e[i] = sum over channels of w_c * (sum of y_c^2 over hop i), whole hops only."""
    x = LR.extent(planes, frames)
    w = np.ones(x.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    assert w.shape == (x.shape[0],)
    h = LR.hop(sr)
    nh = x.shape[1] // h
    e = np.zeros(nh, dtype=np.float64)
    for c in range(x.shape[0]):
        if nh:
            e += w[c] * (LR.weighted(x[c], sr)[:nh * h] ** 2).reshape(nh, h).sum(axis=1)
    return e


def short_term(planes, sr, weights=None, frames=None):
    """(z_st, l_st) of every whole 3 s window, one every 100 ms."""
    e, h = hop_energies(planes, sr, weights, frames), LR.hop(sr)
    J = max(e.size - WINDOW_HOPS + 1, 0)
    z = np.asarray([e[j:j + WINDOW_HOPS].sum() for j in range(J)], dtype=np.float64) / (WINDOW_HOPS * h)
    with np.errstate(divide="ignore"):
        return z, -0.691 + 10.0 * np.log10(z)


def rank(m, fraction):
    """libebur128's nearest-rank index into m ascending values."""
    return int(np.floor((m - 1) * fraction + 0.5))


def measure(planes, sr, weights=None, frames=None):
    """dict(lra, max_momentary, max_short_term, windows, range_margin): the loudness range in LU (0 without a surviving window),
    the two ungated maxima in LUFS (-inf without a block / window), the windows passing both gates and the smallest distance in
    LU of any window from either gate (inf without one)."""
    _, l_m = LR.block_energies(planes, sr, weights, frames)
    z, l = short_term(planes, sr, weights, frames)
    out = dict(lra=0.0, max_momentary=float(np.max(l_m)) if l_m.size else -np.inf,
               max_short_term=float(np.max(l)) if l.size else -np.inf, windows=0,
               range_margin=float(np.min(np.abs(l + 70.0))) if l.size else np.inf)
    keep = l > -70.0
    if not keep.any():
        return out
    gate = -0.691 + 10.0 * np.log10(np.mean(z[keep])) - 20.0
    both = keep & (l > gate)
    out["range_margin"] = min(out["range_margin"], float(np.min(np.abs(l[keep] - gate))))
    s = np.sort(l[both])
    if s.size:
        out.update(lra=float(s[rank(s.size, 0.95)] - s[rank(s.size, 0.10)]), windows=int(s.size))
    return out
