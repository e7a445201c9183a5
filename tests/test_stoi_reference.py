"""CPU checks of the float64 STOI / ESTOI restatement (tests/stoi_reference.py), the oracle of sos_amd.metrics.stoi:
its invariants, its band table and resampler against the published definitions, and its too-short rule."""
import numpy as np
import pytest
import scipy.signal

import stoi_reference as R


@pytest.mark.parametrize("extended", [False, True])
def test_identical_signals_score_one(extended):
    x, _ = R.closed_form_pair(11, 32000, 16000, 0.0)
    assert abs(R.stoi(x, x, 16000, extended) - 1.0) < 1e-9


@pytest.mark.parametrize("extended", [False, True])
def test_scaling_the_processed_signal_changes_nothing(extended):
    x, y = R.closed_form_pair(12, 28000, 14000, 0.05)
    assert abs(R.stoi(x, 3.0 * y.astype(np.float64), 14000, extended) - R.stoi(x, y, 14000, extended)) < 1e-12


def test_third_octave_bands():
    sizes = [2, 2, 3, 3, 5, 5, 7, 9, 12, 14, 18, 22, 29, 36, 45]
    assert [hi - lo for lo, hi in R.BAND_RANGES] == sizes
    assert R.BAND_RANGES[0][0] == 7 and R.BAND_RANGES[-1][1] == 219
    assert all(R.BAND_RANGES[k][1] == R.BAND_RANGES[k + 1][0] for k in range(14))
    assert np.array_equal(R.OBM.sum(axis=1), sizes)
    used = np.flatnonzero(R.OBM.sum(axis=0))
    assert used[0] == 7 and used[-1] == 218 and len(used) == 212


@pytest.mark.parametrize("fs,taps", [(16000, 581), (14000, 509), (8000, 365), (44100, 31947)])
def test_resampler_is_resample_poly_with_the_octave_window(fs, taps):
    h = R.resample_taps(fs)
    assert len(h) == taps and abs(h.sum() - 1.0) < 1e-12
    p, q = R.resample_ratio(fs)
    x = np.random.default_rng(fs).standard_normal(4097)
    want = scipy.signal.resample_poly(x, p, q, window=h)
    got = R.resample_oct(x, fs)
    assert len(got) == len(want) == -(-4097 * p // q)
    assert np.max(np.abs(got - want)) < 1e-12


@pytest.mark.parametrize("n", [0, 100, 256, 257, 4096])
def test_too_few_frames_return_1e5_with_a_warning(n):
    x, y = R.closed_form_pair(13, n, 10000, 0.1)
    with pytest.warns(RuntimeWarning, match="Not enough STFT frames"):
        assert R.stoi(x, y, 10000) == 1e-5
    with pytest.warns(RuntimeWarning):
        assert R.stoi(x, y, 10000, extended=True) == 1e-5


def test_silent_frames_leave_too_few_for_a_score():
    """A long clip that is silent but for 20 loud frames keeps only those: fewer than 30 STFT frames remain."""
    n = 10000 * 3
    x, y = R.closed_form_pair(14, n, 10000, 0.1)
    x[:] = 0.0
    x[12800:12800 + 20 * 128] = 0.5 * np.sin(np.arange(20 * 128) * 0.3)
    with pytest.warns(RuntimeWarning):
        r = R.analyse(x, y, 10000)
    assert r["kept_frames"] <= 22 and r["score"] == 1e-5


@pytest.mark.parametrize("extended", [False, True])
def test_score_falls_as_noise_rises(extended):
    scores = []
    for noise in (0.0, 0.01, 0.03, 0.1, 0.3, 1.0):
        x, y = R.closed_form_pair(15, 32000, 16000, noise)
        scores.append(R.stoi(x, y, 16000, extended))
    assert abs(scores[0] - 1.0) < 1e-9
    assert all(a > b for a, b in zip(scores, scores[1:])), scores
