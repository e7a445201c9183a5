"""tests/mix_reference.py against the oracle it restates, and the preconditions the GPU tests of sos_ragged_mix_f32
(tests/test_gpu_ragged_mix.py) rely on.  CPU only."""
import numpy as np
import pytest

import mix_reference as R
from oracle import frontend as ofe

C = 4096                                                     # SOS_MIX_CHUNK (tests/test_ragged_mix_host_cpu.py pins it)


@pytest.mark.parametrize("snr", [-10, 0, 7])
def test_restatement_equals_the_oracle_on_the_golden_clip(golden, snr):
    g = golden("addsignals")
    want = ofe.add_signals(g["sig"], g["noi"], snr, 0.5)
    got = R.mix(g["sig"], g["noi"], snr)
    for name, w, key in zip(("mixed", "clean", "noise"), want, (f"mixed_{snr}", f"clean_{snr}", f"noise_{snr}")):
        assert np.allclose(got[name], w, atol=1e-7), name
        assert np.allclose(got[name], g[key], atol=1e-7), name
    assert abs(np.max(np.abs(got["mixed"])) - 0.5) < 1e-12 and got["inv"] == 0.5 / got["peak"]
    none = R.mix(g["sig"], g["noi"], snr, norm=None)
    assert none["inv"] == 1.0 and np.array_equal(none["mixed"], none["clean"] + none["noise"])


@pytest.mark.parametrize("noise_len,start,n", [(50, 0, 20), (50, 40, 20), (50, 50, 20), (50, 60, 20), (10, 3, 20), (20, 0, 20),
                                               (0, 0, 5)])
def test_restatement_crops_like_add_noise_to_audio(noise_len, start, n):
    rng = np.random.default_rng(noise_len + start)
    audio, noise = rng.standard_normal(n), rng.standard_normal(noise_len)
    crop = noise[start:start + len(audio)]                   # handoff.add_noise_to_audio, its two lines
    if len(crop) < len(audio):
        crop = np.concatenate((crop, np.zeros(len(audio) - len(crop), dtype=crop.dtype)))
    want = ofe.add_signals(audio, crop, 3.0, 0.5)
    got = R.mix(audio, noise, 3.0, start=start)
    for name, w in zip(("mixed", "clean", "noise"), want):
        assert np.allclose(got[name], w, atol=1e-12), name
    noff, nz = R.crop(noise_len, start, n, n)
    assert nz == min(n, max(noise_len - start, 0)) and 0 <= noff <= noise_len - nz


def test_a_count_limits_the_crop():
    noise = np.arange(1.0, 31.0)
    got = R.mix(np.ones(10), noise, 0.0, start=5, count=4, norm=None)
    assert np.array_equal(got["noise"] != 0, np.arange(10) < 4)
    assert R.crop(30, 5, 4, 10) == (5, 4) and R.crop(30, 28, 100, 10) == (28, 2) and R.crop(30, 5, 0, 10) == (0, 0)


def test_preconditions_of_the_gpu_tests():
    """The fully silenced fixture's oracle mask is all ones; every other fixture has Es > 0, Ez > 0 and peak > 0, so that its
    relative bounds are meaningful, and its clean signal and scaled noise stay within MAX_SPREAD peaks of their sum: the bound
    on the outputs counts f32 roundings relative to that peak (mix_reference.mix), which says nothing where the two cancel."""
    x, z, bits, ratio = R.silenced_case()
    r = R.mix(x, z, 0.0, bits=bits, ratio=ratio)
    assert np.all(r["mask"] == 1.0) and len(r["mask"]) == len(x) and r["Es"] == 0.0 and r["gain"] == 1.0 and r["spread"] == 1.0
    clips, rec, snrs, starts = R.edge_case(C)
    assert [len(c) for c in clips] == [1, 2, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3, 3 * C]
    for x, snr, st in zip(clips, snrs, starts):
        r = R.mix(x, rec, snr, start=st)
        assert r["Es"] > 0 and r["Ez"] > 0 and r["peak"] > 0 and R.crop(len(rec), st, len(x), len(x))[1] == len(x)
        assert r["spread"] <= R.MAX_SPREAD, (len(x), r["spread"])
    clips, noises, snrs, bits, ratios = R.speech_case()
    assert sum(b is None for b in bits) == 1 and sorted({round(14000 / r) for r in ratios if r}) == [25, 30]
    for x, z, snr, b, rt in zip(clips, noises, snrs, bits, ratios):
        assert 0.8 * 14000 <= len(x) <= 2 * 14000
        r = R.mix(x, z, snr, bits=b, ratio=rt)
        assert r["Es"] > 0 and r["Ez"] > 0 and r["peak"] > 0 and r["spread"] <= R.MAX_SPREAD
        if b is not None:
            assert 0 < r["mask"].sum() < len(x)              # silent samples, and others
