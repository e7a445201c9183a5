"""tests/limiter_reference.py held to the properties the rule is built for (CPU): g <= r, so the sample peak of the output meets the
ceiling; g = 1 further than 2 H from any sample over the ceiling; symmetric ramps; window sums that do not depend on the order of
their summands; and what the true-peak form leaves over the ceiling on the fs/4 burst.
Bounds.  Sample form: y = x * (g s) with g <= r = float32(C / a) (1 + 2^-24 at most: the division is rounded once), a = float32(s
|x|) (another 2^-24), g s rounded and the product rounded: (g s) |x| <= C (1 + 3 * 2^-24), y one rounding more.
True form: between two samples the gain is not constant, so the interpolated points of y are not g times those of x.  The slope
of g is at most 1 / (2 H + 1) per sample (one mn leaves the window, one enters, both in [0, 1]) and a point reads 6 samples on
either side with absolute weights summing to S = 1.7251: true peak(y) <= C + (6 / (2 H + 1)) * S * s * max |x|."""
import numpy as np
import pytest

import limiter_reference as M
import r128_reference as R

CEILING = -1.0
S = float(np.max(np.abs(R.true_peak_filter_f32().astype(np.float64)).sum(axis=1)))


def _bursts(seed, ch=2, n=6000):
    """Laplace noise under the ceiling with a few bursts far over it."""
    rng = np.random.default_rng(seed)
    x = 0.03 * rng.laplace(size=(ch, n))
    for at in rng.integers(0, n - 40, size=6):
        x[:, at:at + 40] += 0.5 * rng.laplace(size=(ch, 40))
    return x.astype(np.float32)


@pytest.mark.parametrize("H", (1, 7, 240, 1024))
@pytest.mark.parametrize("true_peak", (False, True))
def test_the_curve_stays_under_the_reduction_and_is_one_away_from_the_peaks(H, true_peak):
    x, s = _bursts(H), np.float32(2.5)
    got = M.limit(x, s, CEILING, H, None, true_peak)
    g, r, C = got["g"], got["r"], M.ceiling(CEILING)
    assert g.dtype == r.dtype == np.float32 and np.all(g <= r) and np.all(g >= M.FLOOR) and np.all(r <= 1.0)
    over = np.flatnonzero(got["p"] * s > C)
    assert over.size and np.array_equal(np.flatnonzero(r < 1.0), over)
    far = np.ones(g.size, bool)
    for t in over:
        far[max(t - 2 * H, 0):t + 2 * H + 1] = False
    assert np.all(g[far] == 1.0) and (far.any() or H == 1024)
    assert got["samples"] == int((g < 1.0).sum()) and got["min_g"] == float(g.min())
    if not true_peak:
        gs = (g * s).astype(np.float64)
        worst = float(np.max(gs * np.abs(x).max(axis=0)) / float(C))
        print("H = %d: largest (g s) |x| / C = 1 %+.3e" % (H, worst - 1.0))
        assert worst <= 1.0 + 3.0 * 2.0 ** -24
        assert np.array_equal(got["y"], x * (g * s)[None, :]) and got["y"].dtype == np.float32


def test_one_peak_gives_symmetric_linear_ramps():
    H, n, at = 50, 1001, 500
    x = np.zeros((1, n), np.float32)
    x[0, at] = 2.0
    got = M.limit(x, 1.0, CEILING, H)
    g, r0 = got["g"], got["r"][at]
    assert np.array_equal(g[at - 2 * H - 5:at + 1], g[at:at + 2 * H + 6][::-1])          # symmetric
    assert np.all(g[:at - 2 * H] == 1.0) and np.all(g[at + 2 * H + 1:] == 1.0) and g[at - 2 * H] < 1.0
    assert g[at] == r0 == np.float32(np.float64(M.ceiling(CEILING)) / 2.0)               # the whole window sits on the peak's minimum
    k = np.arange(0, 2 * H + 1)
    ramp = ((k * np.float64(r0) + (2 * H + 1 - k)) / (2 * H + 1)).astype(np.float32)      # k of the window's 2 H + 1 minima are r0
    assert np.array_equal(g[at - 2 * H - 1 + k], ramp) and np.all(np.diff(g[at - 2 * H - 1:at + 1].astype(np.float64)) < 0)


def test_the_window_sums_do_not_depend_on_the_order():
    rng = np.random.default_rng(5)
    r = M.reduction(np.abs(_bursts(9, 1, 20000))[0], 3.0, M.ceiling(CEILING))
    mn = M.sliding_min(r, 1024).astype(np.float64)
    assert np.all(mn * 2.0 ** 33 == np.round(mn * 2.0 ** 33)) and mn.min() >= 2.0 ** -10   # multiples of 2^-33
    prefix = np.concatenate([[0.0], np.cumsum(mn[:8192])])
    for _ in range(20):
        a = int(rng.integers(0, mn.size - 2049))
        w = mn[a:a + 2049]
        sums = {float(np.sum(w)), float(np.sum(rng.permutation(w))), float(np.sum(np.sort(w))), float(np.sum(np.sort(w)[::-1]))}
        acc = 0.0
        for v in w[::-1]:
            acc += v
        assert sums == {acc}
    assert prefix[2049 + 4000] - prefix[4000] == np.sum(mn[4000:4000 + 2049])


@pytest.mark.parametrize("H", (7, 40, 240))
def test_the_true_form_on_the_quarter_rate_burst(H):
    x, s = R.faded_sine(4, 45.0), np.float32(3.5)
    C = float(M.ceiling(CEILING))
    sample, true = M.limit(x, s, CEILING, H), M.limit(x, s, CEILING, H, None, True)
    bound = C + 6.0 / (2 * H + 1) * S * float(s) * float(np.max(np.abs(x)))
    print("H = %d: true peak %.5f before; %.5f after the sample form (sample peak %.7f), %.5f after the true form; ceiling %.5f, bound %.5f"
          % (H, float(s) * R.true_peak(x), R.true_peak(sample["y"]), np.abs(sample["y"]).max(), R.true_peak(true["y"]), C, bound))
    assert R.true_peak(true["y"]) <= bound
    assert np.abs(sample["y"]).max() <= C * (1.0 + 4.0 * 2.0 ** -24) and R.true_peak(sample["y"]) > 1.05 * C


def test_arguments_of_the_rule():
    assert M.lookahead(5.0, 48000) == 240 and M.lookahead(5.0, 44100) == 220 and M.lookahead(5.0, 200) == 1
    assert M.to_target(-np.inf, -16.0) == 1.0 and M.to_target(-20.0, np.nan) == 1.0 and M.to_target(-20.0, -14.0) == np.float32(10.0 ** 0.3)
    quiet = M.limit(0.01 * np.ones((2, 300), np.float32), 2.0, CEILING, 7)
    assert quiet["samples"] == 0 and quiet["min_g"] == 1.0 and np.array_equal(quiet["y"], np.full((2, 300), np.float32(0.01) * np.float32(2.0)))
    short = M.limit(np.full((1, 10), 3.0, np.float32), 1.0, CEILING, 2, frames=6)
    assert np.all(short["y"][0, 6:] == 3.0) and np.all(short["y"][0, :6] <= M.ceiling(CEILING) * (1.0 + 2.0 ** -22)) and short["g"].size == 6
