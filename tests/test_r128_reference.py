"""tests/r128_reference.py against what is known in closed form: the true peak of a sine is its amplitude wherever its samples
fall, an impulse interpolates to the coefficients themselves, and the loudness range of a sine that steps between two levels is
the level difference.  No GPU."""
import numpy as np
import pytest

import loudness_reference as LR
import r128_reference as R


def test_the_coefficients():
    h = R.true_peak_filter(phase0=True)
    assert h.shape == (4, 12)
    assert h[0][5] == 1.0 and np.allclose(h[0], np.eye(12)[5], rtol=0, atol=1e-16)   # phase 0 is the sample itself (np.sinc(k) ~ 1e-17)
    assert np.allclose(h[1], h[3][::-1], rtol=0, atol=1e-15)                          # h_1[k] = h_3[1 - k]
    assert np.allclose(h[2], h[2][::-1], rtol=0, atol=1e-15)
    assert np.all(np.abs(h[1:].sum(axis=1) - 1.0) < 1e-4)                             # DC gains
    f32 = R.true_peak_filter_f32()
    assert f32.dtype == np.float32 and f32.shape == (3, 12) and np.array_equal(f32, h[1:].astype(np.float32))
    assert abs(float(np.max(np.abs(f32.astype(np.float64)).sum(axis=1))) - 1.7251) < 1e-4


# period in samples, phase in degrees, the sample peak in dBFS
SINES = ((4, 0.0, -6.02), (4, 45.0, -9.03), (6, 60.0, -7.27), (8, 67.5, -6.71))


@pytest.mark.parametrize("period,phase,sample_db", SINES)
def test_the_true_peak_of_a_sine_is_its_amplitude(period, phase, sample_db):
    x = R.faded_sine(period, phase)
    tp = R.db(R.true_peak(x))
    sp = R.db(np.max(np.abs(x)))
    print("fs/%d at %.1f degrees: %.4f dBTP, sample peak %.4f dBFS" % (period, phase, tp, sp))
    assert abs(tp - 20.0 * np.log10(0.5)) <= 0.01
    assert abs(sp - sample_db) <= 0.01
    assert R.true_peak(x) >= float(np.max(np.abs(x)))


def test_an_impulse_reads_exactly_one():
    x = np.zeros((2, 40), np.float32)
    x[1, 17] = -1.0
    assert R.true_peak(x) == 1.0
    v = R.interpolated(x)
    f32 = R.true_peak_filter_f32().astype(np.float64)
    for p in range(3):                                                                # the point n + p / 4 sees the impulse at tap 17 - n
        assert np.array_equal(v[1, 17 - 6 + 1:17 + 6 + 1, p], -f32[p][::-1])
    assert not v[0].any()


def test_frames_crops_and_zero_fills():
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal((2, 50))).astype(np.float32)
    x[0, 30] = 100.0
    assert R.true_peak(x) == 100.0
    assert R.true_peak(x, frames=30) == R.true_peak(x[:, :30]) < 1.0                  # the spike at index `frames` never counts
    assert R.true_peak(x, frames=31) == 100.0
    longer = np.concatenate([x, np.zeros((2, 20), np.float32)], axis=1)
    assert R.true_peak(x, frames=70) == R.true_peak(longer)
    y = np.zeros((1, 8), np.float32)
    y[0, 7] = 1.0                                                                      # rings past the last sample: points up to n = frames - 1
    assert R.interpolated(y).shape == (1, 9, 3) and R.interpolated(y)[0, 8].any()
    assert R.true_peak(np.zeros((1, 0), np.float32)) == 0.0 and R.true_peak(y, frames=0) == 0.0


# stereo 1 kHz sines of 20 s per level: the levels in dBFS -> LRA in LU
STEPS = (((-20.0, -30.0), 10.0), ((-20.0, -15.0), 5.0), ((-40.0, -20.0), 20.0), ((-50.0, -35.0, -20.0, -35.0, -50.0), 15.0))


@pytest.mark.parametrize("sr", [48000, 44100, 8000])
@pytest.mark.parametrize("levels,want", STEPS)
def test_the_range_of_a_stepped_sine_is_the_level_difference(sr, levels, want):
    x = LR.sine(1000.0, sr, [(db, 20.0) for db in levels], channels=2)
    got = R.measure(x, sr)
    print("%d Hz %s: LRA %.6f LU (%d windows)" % (sr, levels, got["lra"], got["windows"]))
    assert abs(got["lra"] - want) <= 0.01
    assert got["windows"] > 0 and got["range_margin"] > 1e-3


def test_short_files():
    sr = 8000
    none = R.measure(LR.sine(1000.0, sr, [(-23.0, 2.5)], channels=2), sr)
    assert (none["windows"], none["lra"], none["max_short_term"]) == (0, 0.0, -np.inf) and none["range_margin"] == np.inf
    assert np.isfinite(none["max_momentary"])
    one = R.measure(LR.sine(1000.0, sr, [(-23.0, 3.0)], channels=2), sr)
    assert (one["windows"], one["lra"]) == (1, 0.0) and np.isfinite(one["max_short_term"])
    tiny = R.measure(LR.sine(1000.0, sr, [(-23.0, 0.3)], channels=2), sr)
    assert tiny["max_momentary"] == -np.inf and tiny["max_short_term"] == -np.inf


def test_the_maxima_of_a_steady_sine_are_its_loudness():
    sr = 48000
    x = LR.sine(1000.0, sr, [(-23.0, 20.0)], channels=2)
    got, ref = R.measure(x, sr), LR.measure(x, sr)
    _, l = LR.block_energies(x, sr)
    assert got["max_momentary"] == float(np.max(l))
    assert abs(got["max_momentary"] - ref["lufs"]) < 0.01 and abs(got["max_short_term"] - ref["lufs"]) < 0.01
    assert abs(got["max_short_term"] + 23.0) < 0.1 and got["lra"] < 0.01


def test_the_tile_python_exports_is_the_kernels():
    """metrics.TRUE_PEAK_TILE restates TP_TILE = TP_THREADS * TP_POINTS of csrc/loudness.hip (the set of exported symbols is
    pinned, so no getter): the edge cases of tests/test_gpu_true_peak.py sit on it, and this keeps the two from drifting apart."""
    import os
    import re
    from sos_amd import metrics
    with open(os.path.join(os.path.dirname(metrics.__file__), "csrc", "loudness.hip")) as fp:
        src = fp.read()
    value = {name: int(v) for name, v in re.findall(r"^#define (TP_THREADS|TP_POINTS) (\d+)", src, re.M)}
    assert re.search(r"^#define TP_TILE \(TP_THREADS \* TP_POINTS\)", src, re.M)
    assert metrics.TRUE_PEAK_TILE == value["TP_THREADS"] * value["TP_POINTS"]
