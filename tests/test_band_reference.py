"""tests/band_reference.py against the rule as include/sos_hip.h states it, and the rule against what it is for: a 12 kHz tone in a
48 / 44.1 kHz recording is gone after the trip through 14 kHz and is back, untouched, after the merge.  CPU only; the resampler
is the oracle's (oracle/wave_io.py, float64)."""
import numpy as np
import pytest

import band_reference as B
from oracle import wave_io as O

SR, HOP = 14000, 158
N, TONE, AMP = 36000, 12000.0, 0.1


def up(v, rate, n):
    """U: v at SR back at `rate`, cut or zero-filled to n frames (resampled below (int64)(len(v) * rho), zero after)."""
    u = O.resample(v, SR, rate)
    out = np.zeros(n)
    out[:min(n, len(u))] = u[:n]
    return out


def amplitude(y, freq, rate, lo, hi):
    """Amplitude of the `freq` component of y[lo:hi] (least squares on sin / cos)."""
    t = np.arange(lo, hi) / rate
    basis = np.stack([np.sin(2 * np.pi * freq * t), np.cos(2 * np.pi * freq * t)], axis=1)
    c, *_ = np.linalg.lstsq(basis, np.asarray(y, dtype=np.float64)[lo:hi], rcond=None)
    return float(np.hypot(*c))


@pytest.fixture(scope="module", params=[48000, 44100])
def trip(request):
    """x = a 12 kHz tone of amplitude 0.1 plus a 1 kHz tone of 0.2; a = x at 14 kHz; m' = the hop multiple the networks return."""
    rate = request.param
    t = np.arange(N) / rate
    x = (AMP * np.sin(2 * np.pi * TONE * t) + 0.2 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)
    a = O.resample(x, rate, SR).astype(np.float32)
    m = len(a)
    assert m == int(np.ceil(N * (float(SR) / rate))) and int(m * (float(rate) / SR)) >= N      # U(a) covers every frame
    mp = HOP * (m // HOP)
    rho = float(rate) / SR
    reach = int(np.ceil(65 * rho))                           # 64 zero crossings of the filter at the low rate, and one sample
    return dict(rate=rate, x=x, a=a, m=m, mp=mp, ua=up(a, rate, N), safe=int(mp * rho) - reach)


def test_identity_returns_the_source(trip):
    """b = a[:m'], g = 1: out = x - U(a) + U(a[:m']) = x wherever no tap of U reaches past m'."""
    out = B.merge(trip["x"], trip["ua"], up(trip["a"][:trip["mp"]], trip["rate"], N), 1.0)
    err = np.max(np.abs(out - trip["x"])[:trip["safe"]])
    print(trip["rate"], "identity: max error", err, "below frame", trip["safe"], "of", N)
    assert trip["safe"] > N - 2 * int(np.ceil(HOP * trip["rate"] / SR)) and err <= 2.0 ** -23 * np.max(np.abs(trip["x"]))


def test_the_plain_round_trip_loses_the_tone_and_keep_returns_it(trip):
    rate, safe = trip["rate"], trip["safe"]
    b = 0.5 * trip["a"][:trip["mp"]]                         # a denoiser that halves what it sees
    ub = up(b, rate, N)
    lo = int(np.ceil(65 * rate / SR))
    lost = amplitude(ub, TONE, rate, lo, safe) / 0.5 / AMP
    kept = amplitude(B.merge(trip["x"], trip["ua"], ub, 1.0), TONE, rate, lo, safe) / AMP
    low = amplitude(B.merge(trip["x"], trip["ua"], ub, 1.0), 1000.0, rate, lo, safe) / 0.2
    print(rate, "12 kHz after 14 kHz and back: %.3g of its amplitude; after 'keep': %.6f; the 1 kHz tone: %.6f" % (lost, kept, low))
    assert lost < 1e-3
    assert abs(kept - 1.0) < 0.01
    assert abs(low - 0.5) < 0.01                             # the low band is the networks' output


def test_follow_scales_the_tone_by_the_low_band_gain(trip):
    rate, safe = trip["rate"], trip["safe"]
    b = 0.25 * trip["a"][:trip["mp"]]
    s = B.gains(trip["a"], b, HOP, 2)
    g = B.interp(s, N, SR, rate, HOP)
    out = B.merge(trip["x"], trip["ua"], up(b, rate, N), g)
    lo = int(np.ceil(65 * rate / SR))
    hi = int((trip["mp"] - 3 * HOP) * rate / SR)             # before the smoothing window reaches the last, empty frame
    assert abs(amplitude(out, TONE, rate, lo, hi) / AMP - 0.25) < 0.01
    assert g[0] == s[0] and min(s[-2:]) <= g[-1] <= max(s[-2:]) and s[-1] < 0.25      # the high band fades out with the low band


def test_a_scaled_copy_gives_its_scale_on_full_frames():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(5 * HOP + 40).astype(np.float32)
    for c in (0.0, 0.3, 1.0, 2.5):
        s = B.gains(a, c * a[:5 * HOP].astype(np.float64), HOP, 0)
        assert s.dtype == np.float32 and s.shape == (6,)
        np.testing.assert_allclose(s[:5], np.float32(min(c, 1.0)), rtol=0, atol=2.0 ** -24)
        assert s[5] == 0.0                                   # the last partial frame has no output of the networks


def test_zero_frames_give_exactly_one_and_zero_output_exactly_zero():
    rng = np.random.default_rng(6)
    a = rng.standard_normal(4 * HOP).astype(np.float32)
    a[HOP:2 * HOP] = 0.0
    b = a.copy()
    b[2 * HOP:3 * HOP] = 0.0
    s = B.gains(a, b, HOP, 0)
    assert s[1] == 1.0 and s[2] == 0.0 and s[0] == 1.0 and s[3] == 1.0
    assert np.array_equal(B.gains(a, np.zeros(0, np.float32), HOP, 0), np.asarray([0, 1, 0, 0], dtype=np.float32))
    assert np.array_equal(B.gains(np.zeros(300, np.float32), np.ones(158, np.float32), HOP, 3), np.ones(2, np.float32))


def test_the_smoothing_window_is_cut_at_both_ends():
    hop = 4
    r = np.asarray([0.5, 1.0, 0.25, 0.0, 0.75, 0.125])
    a = np.ones(len(r) * hop)
    b = np.repeat(r, hop)
    assert np.array_equal(B.gains(a, b, hop, 0), r.astype(np.float32))
    want = [np.mean(r[0:3]), np.mean(r[0:4]), np.mean(r[0:5]), np.mean(r[1:6]), np.mean(r[2:6]), np.mean(r[3:6])]
    assert np.array_equal(B.gains(a, b, hop, 2), np.asarray(want).astype(np.float32))
    assert np.array_equal(B.gains(a, b, hop, 16), np.full(6, np.mean(r), dtype=np.float32))
    for K in (0, 2, 16):                                     # one frame, and it is a partial one
        assert np.array_equal(B.gains(np.ones(3), 0.5 * np.ones(3), hop, K), np.asarray([0.5], dtype=np.float32))
        assert np.array_equal(B.gains(np.ones(3), 0.5 * np.ones(2), hop, K), np.asarray([np.sqrt(0.5 / 3)], dtype=np.float32))


def test_the_interpolation_runs_between_frame_centres_and_clamps():
    s = np.asarray([0.2, 0.8, 0.4], dtype=np.float32).astype(np.float64)
    g = B.interp(s, 40, 1, 3, 4)                             # rho * hop = 12 native frames per low-rate frame
    assert np.all(g[:6] == s[0]) and np.all(g[30:] == s[2])  # p <= 0 up to t = 5.5; p >= 2 from t = 29.5
    p = (np.arange(40) + 0.5) / 12.0 - 0.5
    for t in (6, 11, 17, 18, 29):
        i = int(np.floor(p[t]))
        assert g[t] == s[i] + (p[t] - i) * (s[i + 1] - s[i])
    assert abs(g[17] - 0.8) < 0.6 / 12 and abs(g[18] - 0.8) < 0.4 / 12 and g[6] > s[0] and g[29] > s[2]
    assert np.all(B.interp(s[:1], 40, 1, 3, 4) == s[0])      # J = 1: one value everywhere
    assert np.array_equal(B.merge([1.0, 2.0], [0.5, 0.5], [0.25, 0.25], [0.0, 1.0]), [0.25, 1.75])
