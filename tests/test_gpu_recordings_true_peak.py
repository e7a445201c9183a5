"""recordings.denoise_recordings(peak='true', loudness_range=True) end to end, bf16x3, the closed-form networks and the composition
of tests/test_gpu_recordings_loudness.py.  Three 16-bit files of 2 s in one group under high_band='keep': a mono 44.1 kHz file
whose peak is a 12 ms burst of the fs/4 sine sampled 45 degrees off its crests (11025 Hz lies above 7 kHz, so the merge passes it
to the output as it is), a steady stereo tone at 8 kHz and a steady mono tone at 14 kHz.  The target, -10 LUFS, is loud enough
that the ceiling binds on the burst (crest about 20 dB).  What the closed-form networks make of a steady tone decides whether it
binds there: the byte equality of the two modes is taken from every file that is unbound under both, and one such file must exist.
Bounds.  The written file's true peak (tests/r128_reference.py on the decoded file) under peak='true': at most ceiling * (1 + 2^-24
(g rounded to float32) + 2^-24 (x * g rounded) + 13 * 2^-24 * S (the measured peak, tests/test_gpu_true_peak.py)) + 2^-15 (the 16-bit
rounding moves every sample by at most half a step, the interpolator sums that with gain S = 1.7251: under one step).  Under
peak='sample' the same file is ABOVE the ceiling: the sine alone reads 3.01 dB over; the low band under it is below a tenth of
the burst's amplitude and moves that by less than 1 dB, so more than 2 dB is asserted.  gain_db under 'true' is lower than under
'sample' by the reference's 20 log10(true peak / sample peak), 1e-6 dB.  Range rows: 1e-6 LU of the reference on the composed
planes (tests/test_gpu_loudness_range.py), whose margin is asserted first."""
import numpy as np
import pytest

import loudness_reference as LR
import r128_reference as R
from test_gpu_recordings_loudness import SECONDS, _compose, _container, _encode, _parity_mode, _read, _stored, nets  # noqa: F401

pytestmark = pytest.mark.gpu
TARGET, CEILING = -10.0, -1.0
S = float(np.max(np.abs(R.true_peak_filter_f32().astype(np.float64)).sum(axis=1)))
SPECS = (("burst", 44100, 1), ("steady", 8000, 2), ("tone", 14000, 1))
BASE_KEYS = {"path", "out_path", "channels", "rate", "frames", "format", "clipped", "windows", "loudness_before", "loudness",
             "loudness_target", "gain_db", "peak_limited"}


def _signal(name, rate, ch, seed):
    n = 2 * rate
    t = np.arange(n) / rate
    rng = np.random.default_rng(seed)
    if name == "burst":
        x = 0.02 * np.sin(2 * np.pi * 300.0 * t)[None, :] + 0.001 * rng.standard_normal((ch, n))
        b = R.faded_sine(4, 45.0, amp=0.5, n=529, fade=128)
        x[:, n // 2:n // 2 + b.shape[1]] += b
    else:
        x = np.stack([0.3 * np.sin(2 * np.pi * (440.0 + 60.0 * c) * t + c) for c in range(ch)]) + 0.001 * rng.standard_normal((ch, n))
    return x.astype(np.float32)


def _write(root, name, rate, ch, seed):
    planes = _signal(name, rate, ch, seed)
    data, _ = _encode(planes, "s16")
    path = root / (name + ".wav")
    path.write_bytes(_container(data, "s16", ch, rate))
    return dict(name=name, path=str(path), rate=rate, channels=ch, fmt="s16", frames=planes.shape[1], data=data)


@pytest.fixture(scope="module")
def runs(nets, tmp_path_factory):  # noqa: F811
    import sos_amd
    from sos_amd import recordings
    root = tmp_path_factory.mktemp("tp_in")
    files = [_write(root, *spec, seed=31 + i) for i, spec in enumerate(SPECS)]
    paths = [f["path"] for f in files]
    kw = dict(high_band="keep", loudness=TARGET, peak_ceiling_db=CEILING, **SECONDS)
    out = lambda name: str(tmp_path_factory.mktemp("tp_" + name))                     # noqa: E731
    sos_amd.set_precision("bf16x3")
    try:
        res = dict(omitted=recordings.denoise_recordings(nets[0], nets[1], paths, out("omitted"), **kw),
                   sample=recordings.denoise_recordings(nets[0], nets[1], paths, out("sample"), peak="sample", loudness_range=False, **kw),
                   true=recordings.denoise_recordings(nets[0], nets[1], paths, out("true"), peak="true", loudness_range=True, **kw),
                   source=recordings.denoise_recordings(nets[0], nets[1], paths, out("source"), high_band="keep", loudness="source",
                                                        peak_ceiling_db=CEILING, peak="true", loudness_range=True, **SECONDS))
        planes = _compose(nets, files)
    finally:
        sos_amd.set_precision("bf16")
    return dict(files=files, res=res, planes=planes)


def _written(f, r):
    """The planes a written file decodes to."""
    blob = _read(r["out_path"])
    return _stored(f, blob[len(blob) - 2 * f["frames"] * f["channels"]:])


def test_the_default_mode_is_the_call_without_the_arguments(runs):
    for f, a, b in zip(runs["files"], runs["res"]["omitted"], runs["res"]["sample"]):
        assert _read(a["out_path"]) == _read(b["out_path"]), f["name"]
        assert set(a) == set(b) == BASE_KEYS
        assert {k: v for k, v in a.items() if k != "out_path"} == {k: v for k, v in b.items() if k != "out_path"}


def test_the_true_peak_ceiling_holds_where_the_sample_peak_ceiling_does_not(runs):
    ceiling = 10.0 ** (CEILING / 20.0)
    margin = ceiling * (2.0 ** -24 + 2.0 ** -24 + 13.0 * 2.0 ** -24 * S) + 2.0 ** -15
    bound_both = 0
    for f, a, b in zip(runs["files"], runs["res"]["sample"], runs["res"]["true"]):
        before = LR.extent(runs["planes"][f["name"]], f["frames"])
        tp, sp = R.true_peak(before), float(np.max(np.abs(before)))
        tp_a, tp_b = R.true_peak(_written(f, a)), R.true_peak(_written(f, b))
        print("%s: sample mode %+.4f dB (limited %s) -> %.4f dBTP written; true mode %+.4f dB (limited %s) -> %.4f dBTP written, reported %.4f; "
              "true peak over sample peak %.6f dB, difference of the gains %.9f dB"
              % (f["name"], a["gain_db"], a["peak_limited"], R.db(tp_a), b["gain_db"], b["peak_limited"], R.db(tp_b), b["true_peak_db"],
                 R.db(tp / sp), a["gain_db"] - b["gain_db"]))
        assert tp_b <= ceiling + margin, f["name"]                                     # whatever bound the gain
        assert abs(b["true_peak_db"] - R.db(np.float64(np.float32(10.0 ** (b["gain_db"] / 20.0))) * tp)) <= 20.0 * np.log10(1.0 + 14.0 * 2.0 ** -24 * S)
        if a["peak_limited"] and b["peak_limited"]:
            bound_both += 1
            assert abs((a["gain_db"] - b["gain_db"]) - R.db(tp / sp)) <= 1e-6, f["name"]
        if not a["peak_limited"] and not b["peak_limited"]:
            assert _read(a["out_path"]) == _read(b["out_path"]) and a["gain_db"] == b["gain_db"], f["name"]
    by = {f["name"]: (a, b) for f, a, b in zip(runs["files"], runs["res"]["sample"], runs["res"]["true"])}
    a, b = by["burst"]
    assert a["peak_limited"] and b["peak_limited"] and bound_both >= 1
    burst = runs["files"][0]
    assert R.db(R.true_peak(_written(burst, a))) > CEILING + 2.0                       # about 3 dB over: a QC gate rejects it
    assert R.db(R.true_peak(_written(burst, a))) < CEILING + 3.02
    assert any(not a["peak_limited"] and not b["peak_limited"] for a, b in by.values())         # the byte equality above was exercised


def test_the_rows_are_the_reference_on_the_planes(runs):
    for f, r in zip(runs["files"], runs["res"]["true"]):
        assert set(r) == BASE_KEYS | {"true_peak_db", "lra", "max_momentary", "max_short_term"}
        ref = R.measure(runs["planes"][f["name"]], f["rate"], None, f["frames"])
        lufs = LR.measure(runs["planes"][f["name"]], f["rate"], None, f["frames"])
        assert lufs["margin"] > 1e-6 and ref["range_margin"] >= 1e-3, (f["name"], ref)
        print(f["name"], "LRA %.6f (reference %.6f), max M %.6f S %.6f" % (r["lra"], ref["lra"], r["max_momentary"], r["max_short_term"]))
        assert abs(r["loudness_before"] - lufs["lufs"]) <= 1e-6
        assert abs(r["lra"] - ref["lra"]) <= 1e-6
        assert abs(r["max_momentary"] - (ref["max_momentary"] + r["gain_db"])) <= 1e-6
        assert r["max_short_term"] == -np.inf == ref["max_short_term"]                # 2 s: no 3 s window


def test_source_targets_with_the_true_peak_and_the_range(runs):
    """loudness='source' with both options: the targets are the sources' own loudness (measured apart from the outputs), the extra
    measures are the outputs', and the ceiling is still the true peak's."""
    ceiling = 10.0 ** (CEILING / 20.0)
    margin = ceiling * (2.0 ** -24 + 2.0 ** -24 + 13.0 * 2.0 ** -24 * S) + 2.0 ** -15
    for f, r in zip(runs["files"], runs["res"]["source"]):
        assert set(r) == BASE_KEYS | {"true_peak_db", "lra", "max_momentary", "max_short_term"}
        src, ref = LR.measure(_stored(f), f["rate"]), R.measure(runs["planes"][f["name"]], f["rate"], None, f["frames"])
        assert src["margin"] > 1e-6 and abs(r["loudness_target"] - src["lufs"]) <= 1e-6, f["name"]
        assert abs(r["max_momentary"] - (ref["max_momentary"] + r["gain_db"])) <= 1e-6 and r["lra"] == ref["lra"] == 0.0
        assert R.true_peak(_written(f, r)) <= ceiling + margin, f["name"]
        if not r["peak_limited"]:
            assert abs(r["loudness"] - r["loudness_target"]) <= 1e-6


def test_bad_arguments_are_refused_before_any_launch(runs, nets, tmp_path):  # noqa: F811
    from sos_amd import recordings
    paths = [f["path"] for f in runs["files"]]
    for kw in (dict(peak="true"), dict(peak="true", loudness=None), dict(loudness_range=True), dict(peak="rms", loudness=-23.0), dict(loudness=-23.0, loudness_range="yes"),
               dict(loudness=-23.0, loudness_range=1)):
        with pytest.raises(ValueError):
            recordings.denoise_recordings(nets[0], nets[1], paths, str(tmp_path), **SECONDS, **kw)
    assert not list(tmp_path.iterdir())
