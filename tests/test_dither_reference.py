"""tests/dither_reference.py, the numpy restatement of csrc/dither_core.h, on a CPU: the generator against Random123's published
known answers, and what the dither is for -- the statistics of the total error q - x S on N = 65536 samples (seed 1234, key 7,
S = 2^15).  The bounds are 4 sigma and come from the rule, not from what the reference gave:
  constant input: the error's mean is 0 with sigma sqrt(0.25 / N) = 0.00195 -> |mean| <= 0.008; its variance is 1/12 + 1/6 = 0.25
      whatever the input (triangular dither of 2 LSB makes the first two moments free of the signal) -> 0.25 +- 0.005
  a sine of 0.4 LSB: the projection 2/N sum q sin has sigma 2 sqrt(0.125 / N) = 0.00276 -> 0.4 +- 0.012
  tilt = error power of the lowest quarter of the band over the highest: 'tpdf' is white -> [0.9, 1.1]; 'highpass' has the
      spectrum (1/12)(1 + 2 - 2 cos w): (1 + 0.199) / (1 + 3.801) = 0.250 -> <= 0.3"""
import numpy as np
import pytest

import dither_reference as D
import pcm_reference as R

N, SEED, KEY, S = 65536, 1234, 7, 32768.0


@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % int(v) for v in D.philox4x32_10(counter, key)) == want


def test_word_of_a_sample_follows_the_counter_layout():
    """One block serves four consecutive frames of a channel; frame 2^34 - 1 sits in the block whose counter has a high word."""
    n = np.asarray([0, 1, 2, 3, 4, 2**34 - 4, 2**34 - 1, 2**34], dtype=np.int64)
    w = D.words(n, 3, (5 << 32) | 9, KEY)
    blk0 = D.philox4x32_10([0, 0, 3, KEY], [9, 5])
    assert [int(v) for v in w[:4]] == [int(v) for v in blk0]
    assert int(w[4]) == int(D.philox4x32_10([1, 0, 3, KEY], [9, 5])[0])
    top = D.philox4x32_10([0xFFFFFFFF, 0, 3, KEY], [9, 5])
    assert int(w[5]) == int(top[0]) and int(w[6]) == int(top[3])
    assert int(w[7]) == int(D.philox4x32_10([0, 1, 3, KEY], [9, 5])[0])
    assert int(D.words(n[:1], 2, (5 << 32) | 9, KEY)[0]) != int(w[0])      # another channel, another block


def _error(x, kind):
    """q - x S of a float32 signal with the dither of frames 0 .. N - 1 (kind None: plain rounding)."""
    d = 0.0 if kind is None else D.dither_lsb(kind, np.arange(N), 0, SEED, KEY)
    q, clipped = D.quantise(x, "s16", d)
    assert clipped == 0
    return q, q - x.astype(np.float64) * S


@pytest.mark.parametrize("kind", D.KINDS)
def test_the_dither_is_triangular_on_an_open_interval(kind):
    d = D.dither_lsb(kind, np.arange(N), 0, SEED, KEY)
    assert np.abs(d).max() < 1.0 and abs(d.mean()) <= 4 * np.sqrt(1 / 6 / N)
    assert abs(d.var() - 1 / 6) <= 0.005


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("lsb", [0.0, 0.25, 0.5, 0.75])
def test_constant_inputs_have_an_error_free_of_the_input(kind, lsb):
    x = np.full(N, lsb / S, dtype=np.float32)
    _, e = _error(x, kind)
    print(kind, lsb, "mean", e.mean(), "variance", e.var())
    assert abs(e.mean()) <= 0.008
    assert abs(e.var() - 0.25) <= 0.005


def test_without_dither_the_error_is_the_input():
    x = np.full(N, 0.25 / S, dtype=np.float32)
    q, e = _error(x, None)
    assert not q.any() and e.mean() == -0.25 and e.var() == 0.0


def _sine():
    t = np.arange(N, dtype=np.float64)
    s = np.sin(2 * np.pi * 1024 * t / N)
    return (0.4 / S * s).astype(np.float32), s


def test_a_sine_below_one_lsb_is_gated_to_digital_black_without_dither():
    x, _ = _sine()
    q, _ = _error(x, None)
    assert not q.any()
    assert R.encode(x[None], "s16")[0] == bytes(2 * N)


@pytest.mark.parametrize("kind", D.KINDS)
def test_a_sine_below_one_lsb_survives_with_dither(kind):
    x, s = _sine()
    q, _ = _error(x, kind)
    amplitude = 2.0 / N * float(np.dot(q, s))
    print(kind, "projected amplitude", amplitude)
    assert abs(amplitude - 0.4) <= 0.012


def _tilt(kind):
    x = np.full(N, 0.3 / S, dtype=np.float32)
    _, e = _error(x, kind)
    p = np.abs(np.fft.rfft(e)) ** 2                              # bins 0 .. N / 2; bin 0 holds the mean
    return float(p[1:N // 8 + 1].sum() / p[3 * N // 8:N // 2].sum())


def test_spectral_tilt_of_the_two_kinds():
    flat, high = _tilt("tpdf"), _tilt("highpass")
    print("tilt tpdf", flat, "highpass", high)
    assert 0.9 <= flat <= 1.1
    assert high <= 0.3


def test_encode_is_the_quantiser_over_the_interleaved_frames():
    """encode: crop, dithered zero-fill, interleaving, frame0 and the key; dither=None is pcm_reference.encode."""
    rng = np.random.default_rng(3)
    p = rng.uniform(-1.2, 1.2, size=(3, 9)).astype(np.float32)
    assert D.encode(p, "s16", 7) == R.encode(p, "s16", 7)
    for fmt in D.FORMATS:
        data, clipped = D.encode(p, fmt, 12, "highpass", SEED, KEY, 2**34 - 3)
        got = R.unpack(data, fmt, 3).astype(np.int64) - (128 if fmt == "u8" else 0)
        count = 0
        for c in range(3):
            x = np.concatenate([p[c], np.zeros(3, np.float32)])
            q, k = D.quantise(x, fmt, D.dither_lsb("highpass", np.arange(12) + 2**34 - 3, c, SEED, KEY))
            assert np.array_equal(got[:, c], q), (fmt, c)
            count += k
        assert clipped == count
    whole = D.encode(p, "s24", 9, "tpdf", SEED, KEY, 5)[0]
    parts = b"".join(D.encode(p[:, a:b], "s24", None, "tpdf", SEED, KEY, 5 + a)[0] for a, b in ((0, 1), (1, 8), (8, 9)))
    assert whole == parts                                        # no state: packets with a running frame0
    assert D.encode(p, "s24", 9, "tpdf", SEED + 1, KEY, 5)[0] != whole and D.encode(p, "s24", 9, "tpdf", SEED, KEY + 1, 5)[0] != whole
    with pytest.raises(ValueError):
        D.encode(p, "s32", None, "tpdf")
