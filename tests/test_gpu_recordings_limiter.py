"""recordings.denoise_recordings(limiter='lookahead') end to end: the files, the helpers and the settings of
tests/test_gpu_recordings_true_peak.py (bf16x3, -10 LUFS, -1 dB, three 16-bit files in one group under high_band='keep'; the burst
file's crest of about 20 dB lets the ceiling bind).
Reference: the planes composed from the public pieces, then in numpy the chain the call runs -- tests/limiter_reference.py with
the s the DEVICE derived (audio_io.limit_batch_device on the composed planes reports it; it is held to the reference's 10^((T - L) /
20) within the 1e-6 LU of the measurement and one float32 rounding), tests/loudness_reference.py on the limited planes, the trim
min(1, C / peak) by loudness_reference.gain with the target set to that loudness.
Bounds.  The written file's peak: the margin tests/test_gpu_recordings_true_peak.py derives for the ceiling, for either peak.
Sample mode: the limited planes are the reference's bit for bit, so `loudness` is within the measurement's 1e-6 LU (the gating
margin asserted first) and limiter_samples and limiter_db are equal.  True mode: g is within B = s * 13 * 2^-24 * S * max |x| / C +
2^-23 of the reference's (tests/test_gpu_limiter.py), so every sample within (B / min g + 2^-23) relative; the loudness and the
peak move by no more, the measured true peak by 13 * 2^-24 * S more (tests/test_gpu_true_peak.py): `loudness` within 2 * 20 log10(1 +
B / min g + 14 * 2^-24 * S) + 1e-6, limiter_db within 20 log10(1 + B / min g); limiter_samples differs by at most 4 H + 1 for every
sample whose s p lies within s * 13 * 2^-24 * S * max |x| of the ceiling."""
import numpy as np
import pytest
import torch

import limiter_reference as M
import loudness_reference as LR
import r128_reference as R
from test_gpu_recordings_loudness import SECONDS, _compose, _parity_mode, _read, nets  # noqa: F401
from test_gpu_recordings_true_peak import BASE_KEYS, CEILING, S, SPECS, TARGET, _write, _written

pytestmark = pytest.mark.gpu
MS = 5.0
NEW_KEYS = {"limiter_db", "limiter_samples"}


@pytest.fixture(scope="module")
def runs(nets, tmp_path_factory):  # noqa: F811
    import sos_amd
    from sos_amd import audio_io, metrics, recordings
    root = tmp_path_factory.mktemp("lim_in")
    files = [_write(root, *spec, seed=31 + i) for i, spec in enumerate(SPECS)]
    paths = [f["path"] for f in files]
    kw = dict(high_band="keep", loudness=TARGET, peak_ceiling_db=CEILING, **SECONDS)
    out = lambda name: str(tmp_path_factory.mktemp("lim_" + name))                    # noqa: E731
    call = lambda name, **more: recordings.denoise_recordings(nets[0], nets[1], paths, out(name), **kw, **more)      # noqa: E731
    sos_amd.set_precision("bf16x3")
    try:
        res = {("omitted", "sample"): call("omitted"), ("none", "sample"): call("none", limiter=None),
               ("omitted", "true"): call("plain_true", peak="true", loudness_range=True),
               ("lookahead", "sample"): call("sample", limiter="lookahead", lookahead_ms=MS),
               ("lookahead", "true"): call("true", limiter="lookahead", peak="true", loudness_range=True)}
        planes = _compose(nets, files)
        dev = [torch.from_numpy(planes[f["name"]]).cuda() for f in files]
        rates, frames = [f["rate"] for f in files], [f["frames"] for f in files]
        rows = metrics.loudness_batch(dev, rates, None, frames)["rows"]
        s_dev = audio_io.limit_batch_device(dev, rows, TARGET, CEILING, rates=rates, lookahead_ms=MS, frames=frames)[1][:, 0].cpu().numpy()
    finally:
        sos_amd.set_precision("bf16")
    ref = {}
    for f, s in zip(files, s_dev):
        x, H = planes[f["name"]], M.lookahead(MS, f["rate"])
        before = LR.measure(x, f["rate"], None, f["frames"])
        assert before["margin"] > 1e-6 and abs(R.db(s) - (TARGET - before["lufs"])) <= 1e-6 + R.db(1.0 + 2.0 ** -24), f["name"]
        for mode in ("sample", "true"):
            lim = M.limit(x, s, CEILING, H, f["frames"], mode == "true")
            after = LR.measure(lim["y"], f["rate"], None, f["frames"])
            peak = R.true_peak(lim["y"], f["frames"]) if mode == "true" else after["peak"]
            trim, bound = LR.gain(after["lufs"], peak, after["lufs"], CEILING)
            ext = LR.extent(x, f["frames"])
            ref[(f["name"], mode)] = dict(lim=lim, after=after, trim=float(trim), bound=bound, s=float(s), H=H, before=before["lufs"],
                                          max=float(np.max(np.abs(ext))), written=after["lufs"] + R.db(trim))
    return dict(files=files, res=res, ref=ref)


def test_none_is_the_call_without_the_argument(runs):
    for f, a, b in zip(runs["files"], runs["res"][("omitted", "sample")], runs["res"][("none", "sample")]):
        assert _read(a["out_path"]) == _read(b["out_path"]), f["name"]
        assert set(a) == set(b) == BASE_KEYS
        assert {k: v for k, v in a.items() if k != "out_path"} == {k: v for k, v in b.items() if k != "out_path"}


@pytest.mark.parametrize("mode", ("sample", "true"))
def test_the_ceiling_holds_and_the_rows_are_the_reference(runs, mode):
    ceiling = 10.0 ** (CEILING / 20.0)
    margin = ceiling * (2.0 ** -24 + 2.0 ** -24 + 13.0 * 2.0 ** -24 * S) + 2.0 ** -15
    for f, r in zip(runs["files"], runs["res"][("lookahead", mode)]):
        ref = runs["ref"][(f["name"], mode)]
        assert set(r) == BASE_KEYS | NEW_KEYS | ({"true_peak_db", "lra", "max_momentary", "max_short_term"} if mode == "true" else set())
        y = _written(f, r)
        peak = R.true_peak(y) if mode == "true" else float(np.max(np.abs(y)))
        lim, after = ref["lim"], ref["after"]
        print("%s (%s): s %+.4f dB, limiter %.4f dB over %d samples (reference %.4f, %d), trim %+.2e dB (limited %s), written peak %.5f (ceiling %.5f), "
              "loudness %.6f (reference %.6f, target %.1f)" % (f["name"], mode, R.db(ref["s"]), r["limiter_db"], r["limiter_samples"], R.db(lim["min_g"]),
                                                             lim["samples"], r["gain_db"] - R.db(ref["s"]), r["peak_limited"], peak, ceiling,
                                                             r["loudness"], ref["written"], TARGET))
        assert peak <= ceiling + margin, f["name"]
        assert after["margin"] > 1e-6 and r["limiter_db"] <= 0.0 and r["loudness_target"] == TARGET
        assert abs(r["loudness_before"] - ref["before"]) <= 1e-6
        if mode == "sample":
            assert abs(r["loudness"] - ref["written"]) <= 1e-6 and r["limiter_samples"] == lim["samples"], f["name"]
            assert abs(r["limiter_db"] - R.db(lim["min_g"])) <= 1e-9 and r["peak_limited"] == ref["bound"]
            assert abs(r["gain_db"] - (R.db(ref["s"]) + R.db(ref["trim"]))) <= 1e-6
        else:
            delta = 13.0 * 2.0 ** -24 * S * ref["max"]
            rel = (ref["s"] * delta / ceiling + 2.0 ** -23) / lim["min_g"]
            assert abs(r["loudness"] - ref["written"]) <= 2.0 * R.db(1.0 + rel + 14.0 * 2.0 ** -24 * S) + 1e-6, f["name"]
            assert abs(r["limiter_db"] - R.db(lim["min_g"])) <= R.db(1.0 + rel)
            near = int(np.sum(np.abs(lim["p"].astype(np.float64) * ref["s"] - ceiling) <= ref["s"] * delta))
            assert abs(r["limiter_samples"] - lim["samples"]) <= near * (4 * ref["H"] + 1), (f["name"], near)
            assert abs(r["true_peak_db"] - R.db(peak)) <= 0.01                        # the 16-bit rounding on a peak near 0.89
            measured = R.measure(lim["y"], f["rate"], None, f["frames"])
            assert abs(r["max_momentary"] - (measured["max_momentary"] + R.db(ref["trim"]))) <= 2.0 * R.db(1.0 + rel + 14.0 * 2.0 ** -24 * S) + 1e-6


@pytest.mark.parametrize("mode", ("sample", "true"))
def test_the_burst_comes_closer_to_its_target_and_unbound_files_keep_their_bytes(runs, mode):
    plain, limited = runs["res"][("omitted", mode)], runs["res"][("lookahead", mode)]
    same = 0
    for f, a, b in zip(runs["files"], plain, limited):
        print("%s (%s): without %.4f LUFS (peak-limited %s), with %.4f LUFS (limiter %.2f dB, trim engaged %s); target %.1f"
              % (f["name"], mode, a["loudness"], a["peak_limited"], b["loudness"], b["limiter_db"], b["peak_limited"], TARGET))
        if f["name"] == "burst":
            assert a["peak_limited"] and abs(b["loudness"] - TARGET) < abs(a["loudness"] - TARGET) and b["limiter_samples"] > 0
        if not a["peak_limited"]:
            same += 1
            assert _read(a["out_path"]) == _read(b["out_path"]) and b["limiter_samples"] == 0 and b["limiter_db"] == 0.0, f["name"]
            assert not b["peak_limited"] and abs(b["gain_db"] - a["gain_db"]) <= 1e-6
    assert same >= 1


def test_bad_arguments_are_refused_with_nothing_written(runs, nets, tmp_path):  # noqa: F811
    from sos_amd import recordings
    paths = [f["path"] for f in runs["files"]]
    for kw in (dict(limiter="brickwall", loudness=TARGET), dict(limiter="lookahead"), dict(limiter="lookahead", loudness=None),
               dict(limiter="lookahead", loudness=TARGET, lookahead_ms=0.0), dict(limiter="lookahead", loudness=TARGET, lookahead_ms=float("inf")),
               dict(limiter="lookahead", loudness=TARGET, lookahead_ms="5"), dict(loudness=TARGET, lookahead_ms=-1.0),
               dict(limiter="lookahead", loudness=TARGET, lookahead_ms=30.0), dict(limiter="lookahead", loudness=TARGET, lookahead_ms=0.05)):
        with pytest.raises(ValueError) as e:
            recordings.denoise_recordings(nets[0], nets[1], paths, str(tmp_path), **SECONDS, **kw)
        if kw.get("lookahead_ms") in (30.0, 0.05):
            assert paths[0 if kw["lookahead_ms"] == 30.0 else 1] in str(e.value)      # 1323 samples at 44.1 kHz, 0 at 8 kHz
    assert not list(tmp_path.iterdir())
