"""handoff.denoise_first_model(window_seconds=): the files of pred_data.json through overlapping windows, the four signals of
every file cross-faded by one sos_window_stitch_planes_f32 launch into a file-major buffer.  bf16x3, the closed-form denoiser,
cores of 80 hops and contexts of 8 hops as in tests/test_gpu_window.py.  Bounds: WAVE files of one-window files and of
max_batch=1 runs byte for byte; the default grouping within 2e-4 of the file's peak (the ragged-versus-alone bound of
tests/test_gpu_pipeline.py in bf16x3); stitched samples bit for bit outside the overlap zones and within R.stitch_bound inside
(tests/window_reference.py, float64); measures within 1e-9 relative (METRIC_RTOL of tests/test_gpu_handoff_files_batch.py)."""
import json
import os

import numpy as np
import pytest
import torch

import window_reference as R
from oracle import nets as onet

pytestmark = pytest.mark.gpu
METRIC_RTOL = 1e-9
WAVE_TOL = 2e-4
HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
SECONDS = dict(window_seconds=CORE / 14000, context_seconds=CONTEXT / 14000)
WAVES = ("noisy_input", "noise_intervals", "predicted_full_noise", "denoised_output")
GT_WAVES = ("ground_truth_full_noise", "ground_truth_clean_input")
METRIC_KEYS = ("l1", "stoi", "csig", "cbak", "covl", "pesq", "ssnr_regular", "ssnr_shift", "ssnr_clip", "ssnr_exsi", "overall_snr")
# name, samples as stored, framerate, stored rate: three windows, two windows, one window (resampled to 14 kHz), one window
SPECS = (("a", 3 * CORE + 5 * HOP + 77, 30, 14000), ("b", 28000, 25, 14000), ("c", 27200, 30, 16000), ("d", 11200, 30, 14000))
WINDOWS = dict(a=3, b=2, c=1, d=1)


def _pesq(clean, output, sr):
    return 2.5


@pytest.fixture(autouse=True)
def _parity_mode():
    import sos_amd
    sos_amd.set_precision("bf16x3")
    try:
        yield
    finally:
        sos_amd.set_precision("bf16")


def _denoiser():
    from sos_amd.common import MyConfig
    from sos_amd.denoiser import networks as jnet
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    return jm.cuda().eval()


def _fixture(root, specs=SPECS):
    """pred_data_snr10.json with clean_audio / full_noise entries, written with audio_io.write_wav like
    test_gpu_handoff_files_batch._fixture, the files given by their sample counts."""
    from sos_amd import audio_io
    (root / "recovered").mkdir(parents=True)
    rng = np.random.default_rng(19)
    files = []
    for name, n, fr, rate in specs:
        nfr = int(round(fr * n / rate))
        t = np.arange(n) / rate
        clean = (0.3 * np.sin(2 * np.pi * 300 * t) * (0.2 + (np.sin(2 * np.pi * 1.3 * t) > -0.4))
                 + 0.003 * rng.standard_normal(n)).astype(np.float32)
        noise = (0.05 * rng.standard_normal(n)).astype(np.float32)
        for suffix, sig in (("_clean", clean), ("_full_noise", noise), ("_mixed", clean + noise)):
            audio_io.write_wav(str(root / "recovered" / (name + suffix + ".wav")), sig, rate)
        bits = "".join("1" if (i // 10) % 3 else "0" for i in range(nfr))
        gt = "".join("0" if (i // 7) % 4 == 1 else "1" for i in range(nfr))
        files.append(dict(path="/a/%s.wav" % name, framerate=fr, bit_stream=gt, recovered_prediction=bits,
                          mixed_audio="recovered/%s_mixed.wav" % name, clean_audio="recovered/%s_clean.wav" % name,
                          full_noise="recovered/%s_full_noise.wav" % name))
    pd = dict(dataset_path="/a", num_videos=len(files), data_total_frames=60, data_center_frames=1, sigmoid_threshold=0.5,
              snr=10, files=files)
    path = root / "pred_data_snr10.json"
    with open(path, "w") as fp:
        json.dump(pd, fp)
    return str(path)


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """The whole-file run (one file per group), the windowed run with one window per group and the windowed run with the
    default grouping, each with and without known clean signals: computed once in bf16x3 and left unchanged."""
    import sos_amd
    from sos_amd import handoff
    root = tmp_path_factory.mktemp("handoff_long")
    path = _fixture(root / "m1")
    jm = _denoiser()
    with open(path) as fp:
        files = json.load(fp)["files"]
    res = dict(json=path, jm=jm, root=root, files=files)
    sos_amd.set_precision("bf16x3")
    try:
        for known in (True, False):
            tag = "known" if known else "unknown"
            kw = dict(sr=14000, snr=10, unknown_clean_signal=not known, stoi_fn=True, pesq_fn=_pesq)
            res["whole_" + tag] = handoff.denoise_first_model(jm, path, str(root / ("whole_" + tag)), max_batch=1, **kw)
            res["alone_" + tag] = handoff.denoise_first_model(jm, path, str(root / ("alone_" + tag)), max_batch=1, **SECONDS, **kw)
            res["grouped_" + tag] = handoff.denoise_first_model(jm, path, str(root / ("grouped_" + tag)), **SECONDS, **kw)
    finally:
        sos_amd.set_precision("bf16")
    return res


def _wave(path):
    from sos_amd import audio_io
    return audio_io.read_wave(path)


def _bytes(path):
    with open(path, "rb") as fp:
        return fp.read()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_plan_of_the_files():
    assert [len(R.plan([n * 14000 // rate], CORE, CONTEXT)) for _, n, _, rate in SPECS] == [3, 2, 1, 1]


@pytest.mark.parametrize("tag", ["known", "unknown"])
@pytest.mark.parametrize("run", ["alone", "grouped"])
def test_keys_layout_and_headers_are_the_whole_file_runs(chain, run, tag):
    whole, got = chain["whole_" + tag], chain[run + "_" + tag]
    names = WAVES + (GT_WAVES if tag == "known" else ())
    assert [b["id"] for b in got] == ["a", "b", "c", "d"] and len(whole) == 4
    want_keys = ["id", "path"] + (["clean_audio_path"] if tag == "known" else []) + ["mixed_audio_path"] + \
        (["full_noise_path"] if tag == "known" else []) + ["bitstream", "sr", "snr"] + (list(METRIC_KEYS) if tag == "known" else []) + list(names)
    for a, b in zip(whole, got):
        assert list(a) == list(b) == want_keys
        for k in a:
            if k in names:
                assert os.path.basename(b[k]) == k + ".wav" and os.path.basename(os.path.dirname(b[k])) == a["id"]
                assert os.path.basename(os.path.dirname(os.path.dirname(b[k]))) == "snr10"
                (wa, ka, ra), (wb, kb, rb) = _wave(a[k]), _wave(b[k])
                assert (ka, ra, wa.shape, wa.dtype) == (kb, rb, wb.shape, wb.dtype), (a["id"], k)
                assert len(_bytes(a[k])) == len(_bytes(b[k]))
            elif k in METRIC_KEYS:
                assert type(a[k]) is type(b[k]), (k, type(a[k]), type(b[k]))
            else:
                assert a[k] == b[k] and type(a[k]) is type(b[k]), k
        assert sorted(os.listdir(os.path.dirname(b["denoised_output"]))) == sorted(os.listdir(os.path.dirname(a["denoised_output"])))
        with open(os.path.join(os.path.dirname(b["denoised_output"]), "stat.json")) as fp:
            assert json.load(fp) == json.loads(json.dumps(b))
    ev = []
    for d in ("whole_" + tag, run + "_" + tag):
        with open(os.path.join(str(chain["root"] / d), "eval_results_snr10.json")) as fp:
            ev.append(json.load(fp))
    assert list(ev[0]) == list(ev[1]) and [list(f) for f in ev[0]["files"]] == [list(f) for f in ev[1]["files"]]
    assert ("denoise_statistics" in ev[1]) == (tag == "known")
    if tag == "known":
        assert list(ev[1]["denoise_statistics"]) == ["avg_" + k for k in METRIC_KEYS] == list(ev[0]["denoise_statistics"])
    assert {k: v for k, v in ev[0].items() if k not in ("files", "denoise_statistics")} == \
        {k: v for k, v in ev[1].items() if k not in ("files", "denoise_statistics")}
    assert ev[1]["files"] == json.loads(json.dumps(got))


@pytest.mark.parametrize("tag", ["known", "unknown"])
def test_one_window_files_are_the_whole_file_runs_byte_for_byte(chain, tag):
    names = WAVES + (GT_WAVES if tag == "known" else ())
    for a, b in zip(chain["whole_" + tag], chain["alone_" + tag]):
        if WINDOWS[a["id"]] == 1:
            for k in names:
                assert _bytes(a[k]) == _bytes(b[k]), (a["id"], k)
        else:
            assert _bytes(a["denoised_output"]) != _bytes(b["denoised_output"]), a["id"]      # windows approximate the whole file


@pytest.mark.parametrize("tag", ["known", "unknown"])
def test_long_files_are_denoise_longs_four_signals_byte_for_byte(chain, tag, tmp_path):
    from sos_amd import audio_io, pipeline
    for d, b in zip(chain["files"], chain["alone_" + tag]):
        if WINDOWS[b["id"]] == 1:
            continue
        wave, _ = audio_io.load_device(b["mixed_audio_path"], sr=14000)
        bits = np.asarray([0 if c == "0" else 1 for c in d["recovered_prediction"]], dtype=np.uint8)
        outs, extra = pipeline.denoise_long(None, chain["jm"], [wave], fps=d["framerate"], bits=[bits], signals=True, max_batch=1,
                                            **SECONDS)
        for k, sig in zip(WAVES, (extra[0]["noisy_input"], extra[0]["noise_intervals"], extra[0]["predicted_full_noise"], outs[0])):
            p = str(tmp_path / (b["id"] + k + ".wav"))
            audio_io.write_wav(p, sig.cpu().numpy(), 14000)
            assert _bytes(p) == _bytes(b[k]), (b["id"], k)


@pytest.mark.parametrize("tag", ["known", "unknown"])
def test_the_default_grouping_is_within_the_ragged_bound_of_one_window_per_group(chain, tag):
    names = WAVES + (GT_WAVES if tag == "known" else ())
    for a, b in zip(chain["alone_" + tag], chain["grouped_" + tag]):
        for k in names:
            wa, wb = _wave(a[k])[0], _wave(b[k])[0]
            err = float(np.abs(wa - wb).max() / np.abs(wa).max())
            print(tag, a["id"], k, "samples", wa.shape[0], "max |diff| / peak %.3e" % err)
            assert wa.shape == wb.shape and err < WAVE_TOL, (a["id"], k, err)


def test_ground_truth_files_of_long_files_are_the_stitched_round_trips_of_host_cut_windows(chain):
    """ground_truth_full_noise / ground_truth_clean_input of the files of several windows (one window per group): the float64
    stitch of the STFT -> ISTFT round trips of the windows cut on the host -- of `full_noise`, and of the clean recording
    silenced on its ground-truth silent intervals at full length (wave - wave * mask, M2/predict.py:321)."""
    from sos_amd import audio_io, engine as E, tools, transform
    for d, b in zip(chain["files"], chain["alone_known"]):
        if WINDOWS[b["id"]] == 1:
            continue
        noise, _ = audio_io.load_device(b["full_noise_path"], sr=14000)
        clean, _ = audio_io.load_device(b["clean_audio_path"], sr=14000)
        gt = torch.from_numpy(np.asarray([0 if c == "0" else 1 for c in d["bit_stream"]], dtype=np.uint8)).cuda()
        _, masked = tools.bits_to_mask_batch(gt[None], 14000.0 / d["framerate"], clean.numel(), clean[None])
        silenced = clean - masked[0]
        n_out = HOP * (noise.numel() // HOP)
        for key, x in (("ground_truth_full_noise", noise), ("ground_truth_clean_input", silenced)):
            wins = R.plan([x.numel()], CORE, CONTEXT)
            assert len(wins) == WINDOWS[b["id"]]
            rows = []
            for w in wins:
                rag = E.Ragged([1 + w.samples // HOP], x.device, n_samples=[w.samples])
                cut = x[w.start:w.start + w.samples][None].contiguous()
                y = transform.istft_batch(transform.stft_batch(cut, clip_samples=rag.tab([w.samples])), clip_frames=rag.level(0))
                rows.append(y[0, :HOP * (w.samples // HOP)].cpu().numpy())
            want, blended = R.stitch(wins, rows, CONTEXT)
            bound = R.stitch_bound(wins, rows, CONTEXT)
            got, kind, rate = _wave(b[key])
            got = np.asarray(got).reshape(-1)
            assert rate == 14000 and got.dtype == np.float32 and got.shape == (n_out,) == want.shape
            assert _same_bits(got[~blended], want[~blended].astype(np.float32)), (b["id"], key)
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err[blended] <= bound[blended]), (b["id"], key, float((err[blended] / np.maximum(bound[blended], 1e-300)).max()))
            assert blended.sum() == 2 * CONTEXT * (len(wins) - 1) and np.abs(got).max() > 0


@pytest.mark.parametrize("run", ["alone", "grouped"])
def test_measures_are_those_of_the_files_the_run_wrote(chain, run):
    from sos_amd import audio_io, metrics
    for b in chain[run + "_known"]:
        out, _ = audio_io.load_device(b["denoised_output"], sr=None)
        clean, _ = audio_io.load_device(b["ground_truth_clean_input"], sr=None)
        out16, clean16 = audio_io.resample_device(out, 14000, 16000), audio_io.resample_device(clean, 14000, 16000)
        n = min(out16.numel(), clean16.numel())
        want = metrics.evaluate_metrics(out16[:n], clean16[:n], sr=16000, pesq=2.5, stoi=None)
        for k in METRIC_KEYS:
            print(run, b["id"], k, b[k], want[k])
            if k == "stoi":
                assert isinstance(b[k], float) and 0 < b[k] < 1
                assert abs(b[k] - metrics.stoi(clean16[:n].cpu().numpy(), out16[:n].cpu().numpy(), 16000)) <= METRIC_RTOL * b[k]
                continue
            assert isinstance(b[k], float) and abs(b[k] - want[k]) <= METRIC_RTOL * abs(want[k]), (b["id"], k, b[k], want[k])


def test_a_short_file_and_bad_windows_are_refused_before_anything_is_written(chain, tmp_path):
    from sos_amd import handoff
    jm = chain["jm"]
    short = _fixture(tmp_path / "short", specs=(("c", 28000, 30, 14000), ("tiny", 62 * HOP, 30, 14000)))         # 63 STFT frames
    with pytest.raises(ValueError, match="tiny_mixed.wav"):
        handoff.denoise_first_model(jm, short, str(tmp_path / "out_short"), sr=14000, snr=10, **SECONDS)
    assert not os.path.exists(str(tmp_path / "out_short"))
    with pytest.raises(ValueError):
        handoff.denoise_first_model(jm, chain["json"], str(tmp_path / "out_args"), sr=14000, snr=10, window_seconds=1.0,
                                    context_seconds=0.6)
    assert not os.path.exists(str(tmp_path / "out_args"))
