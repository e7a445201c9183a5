"""Pins tests/sdr_reference.py, the float64 oracle of sos_amd.metrics.si_sdr / sdr (CPU only): the three ways to the
BSS-eval SDR (LU on the lag matrix, mir_eval's explicit decomposition, the Levinson recursion the kernel runs) agree and give
the recorded values; SI-SDR is the project's oracle formula; both are scale invariant; SDR >= SI-SDR, by far on a filtered
estimate."""
import numpy as np
import pytest

import sdr_reference as R
from oracle import frontend as ofe


@pytest.mark.parametrize("row", R.TABLE, ids=[f"idx{r[0]}" for r in R.TABLE])
def test_three_forms_agree_on_the_recorded_values(row):
    x, y = R.table_pair(row)
    a, b, c = R.sdr(x, y), R.sdr_explicit(x, y), R.sdr_levinson(x, y)
    assert abs(a - b) < 1e-8 and abs(a - c) < 1e-8, (a, b, c)
    assert abs(a - row[4]) < 1e-6, (a, row[4])                  # the recorded value has six decimals
    assert a >= R.si_sdr(x, y)                                  # lag 0 is in the span


def test_analyse_reports_what_the_table_says():
    x, y = R.table_pair(R.TABLE[0])
    a = R.analyse(x, y)
    assert a["score"] == R.sdr(x, y)
    assert 3e5 < a["cond"] < 5e5 and abs(a["one_minus_p_over_e"] - 2.6e-2) < 1e-3 and a["lu_minus_levinson_db"] < 1e-10
    r, d, e = R.correlations(x, y, 8)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    assert r[3] == np.dot(x64[:-3], x64[3:]) and d[5] == np.dot(x64[:-5], y64[5:]) and e == np.dot(y64, y64)


@pytest.mark.parametrize("zero_mean", [False, True])
def test_si_sdr_is_the_oracle_formula(zero_mean):
    x, y = R.table_pair(R.TABLE[3])
    x = x + np.float32(0.01)                                    # a mean worth removing
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    want = ofe.si_sdr(y64 - np.mean(y64), x64 - np.mean(x64)) if zero_mean else ofe.si_sdr(y, x)
    assert R.si_sdr(x, y, zero_mean) == want
    assert R.si_sdr(x, y, True) != R.si_sdr(x, y, False)


def test_both_measures_are_scale_invariant():
    x, y = R.table_pair(R.TABLE[0])
    ys = 0.3 * y.astype(np.float64)
    assert abs(R.sdr(x, ys) - R.sdr(x, y)) < 1e-9
    assert abs(R.si_sdr(x, ys) - R.si_sdr(x, y)) < 1e-9


def test_filtered_estimate_scores_far_higher_in_sdr_than_in_si_sdr():
    x, y = R.filtered_pair(33, 48000, 16000)
    a, s = R.sdr(x, y), R.si_sdr(x, y)
    assert a > s + 10, (a, s)
    assert R.sdr(x, y, 64) < a - 10                             # the taps at 150 are outside a 64-tap span


def test_short_and_degenerate_clips():
    from stoi_reference import closed_form_pair
    for n in (511, 512, 2000):
        x, y = closed_form_pair(23, n, 16000, 0.1)
        a = R.analyse(x, y)
        assert np.isfinite(a["score"]) and a["lu_minus_levinson_db"] < 1e-9 and a["score"] >= R.si_sdr(x, y)
    x, y = closed_form_pair(21, 32000, 16000, 0.05)
    assert R.sdr(x, x) == float("inf") or R.sdr(x, x) >= 100
    assert np.isnan(R.sdr_levinson(np.zeros(1000), y[:1000]))
    assert np.isfinite(R.si_sdr(np.zeros(1000), y[:1000]))
    with pytest.raises(ValueError):
        R.sdr(x, y[:-1])
