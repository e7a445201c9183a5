"""handoff.denoise_files(batch_metrics=True): the objective measures of all files from one batched resampling and one
evaluate_metrics_batch, against the per-file path on the same network and data -- same keys in the same order, the same
files byte for byte, the measures within the batch-versus-loop bound of tests/test_gpu_metrics_batch.py (1e-9 relative:
the batch adds its f64 frame sums in another order than the one-clip kernels), STOI equal."""
import json
import os

import numpy as np
import pytest

from oracle import nets as onet
from test_gpu_handoff import _make_dataset

pytestmark = pytest.mark.gpu
METRIC_RTOL = 1e-9
WAVES = ("noisy_input", "noise_intervals", "predicted_full_noise", "denoised_output")
GT_WAVES = ("ground_truth_full_noise", "ground_truth_clean_input")
METRIC_KEYS = ("l1", "stoi", "csig", "cbak", "covl", "pesq", "ssnr_regular", "ssnr_shift", "ssnr_clip", "ssnr_exsi", "overall_snr")


def _net():
    from sos_amd.common import MyConfig
    from sos_amd.denoiser import networks as jnet
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    return jm.cuda().eval()


def _known_clean_fixture(root):
    """pred_data_snr10.json with clean_audio / full_noise entries, as tests/test_gpu_handoff.py builds it for one file; here
    three files of different lengths."""
    from sos_amd import audio_io
    (root / "recovered").mkdir(parents=True)
    rng = np.random.default_rng(9)
    files = []
    for name, secs in (("c", 2.0), ("d", 1.3), ("e", 1.7)):
        n, nfr = int(14000 * secs), int(round(30 * secs))
        t = np.arange(n) / 14000
        clean = (0.3 * np.sin(2 * np.pi * 300 * t) * (0.2 + (np.sin(2 * np.pi * 1.3 * t) > -0.4))
                 + 0.003 * rng.standard_normal(n)).astype(np.float32)
        noise = (0.05 * rng.standard_normal(n)).astype(np.float32)
        for suffix, sig in (("_clean", clean), ("_full_noise", noise), ("_mixed", clean + noise)):
            audio_io.write_wav(str(root / "recovered" / (name + suffix + ".wav")), sig, 14000)
        bits = "".join("1" if (i // 10) % 3 else "0" for i in range(nfr))
        files.append(dict(path="/a/%s.wav" % name, framerate=30, bit_stream="1" * nfr, recovered_prediction=bits,
                          mixed_audio="recovered/%s_mixed.wav" % name, clean_audio="recovered/%s_clean.wav" % name,
                          full_noise="recovered/%s_full_noise.wav" % name))
    pd = dict(dataset_path="/a", num_videos=len(files), data_total_frames=60, data_center_frames=1, sigmoid_threshold=0.5,
              snr=10, files=files)
    path = root / "pred_data_snr10.json"
    with open(path, "w") as fp:
        json.dump(pd, fp)
    return str(path)


def _read(path):
    with open(path, "rb") as fp:
        return fp.read()


def _same_files(a, b, names):
    for name in names:
        assert os.path.basename(a[name]) == os.path.basename(b[name]) == name + ".wav"
        assert os.path.basename(os.path.dirname(a[name])) == os.path.basename(os.path.dirname(b[name])) == a["id"]
        assert _read(a[name]) == _read(b[name]), (a["id"], name)


def test_batched_measures_equal_the_per_file_path(tmp_path):
    from sos_amd import handoff, metrics
    dli = handoff.get_data_from_first_model(_known_clean_fixture(tmp_path / "m1"), sr=14000, unknown_clean_signal=False)
    assert len({item["mixed"].shape[-1] for item in dli[0]}) == 3          # three different lengths
    jm = _net()
    pesq_fn = lambda c, o, sr: 2.5                                         # noqa: E731
    loop_dir, batch_dir = str(tmp_path / "loop"), str(tmp_path / "batch")
    loop = handoff.denoise_files(jm, dli, loop_dir, snr=10, stoi_fn=metrics.stoi, pesq_fn=pesq_fn)
    batch = handoff.denoise_files(jm, dli, batch_dir, snr=10, stoi_fn=True, pesq_fn=pesq_fn, batch_metrics=True)
    assert len(loop) == len(batch) == 3
    for a, b in zip(loop, batch):
        assert list(a) == list(b)
        assert list(a)[8:19] == list(METRIC_KEYS)
        for k in ("id", "path", "clean_audio_path", "mixed_audio_path", "full_noise_path", "bitstream", "sr", "snr"):
            assert a[k] == b[k] and type(a[k]) is type(b[k]), k
        for k in METRIC_KEYS:
            print(a["id"], k, a[k], b[k])
            assert type(a[k]) is type(b[k]) and isinstance(a[k], float), (k, type(a[k]), type(b[k]))
            assert abs(a[k] - b[k]) <= METRIC_RTOL * abs(a[k]), (a["id"], k, a[k], b[k])
        assert a["stoi"] == b["stoi"] and 0 < b["stoi"] < 1 and b["pesq"] == 2.5
        _same_files(a, b, WAVES + GT_WAVES)
        with open(os.path.join(os.path.dirname(b["denoised_output"]), "stat.json")) as fp:
            assert json.load(fp) == json.loads(json.dumps(b))
    ev = []
    for d in (loop_dir, batch_dir):
        with open(os.path.join(d, "eval_results_snr10.json")) as fp:
            ev.append(json.load(fp))
    assert list(ev[0]) == list(ev[1]) and list(ev[0]["denoise_statistics"]) == list(ev[1]["denoise_statistics"])
    assert list(ev[1]["denoise_statistics"]) == ["avg_" + k for k in METRIC_KEYS]
    for k, v in ev[0]["denoise_statistics"].items():
        w = ev[1]["denoise_statistics"][k]
        assert type(v) is type(w) and isinstance(v, float) and abs(v - w) <= METRIC_RTOL * abs(v), (k, v, w)
    assert [list(f) for f in ev[0]["files"]] == [list(f) for f in ev[1]["files"]]
    # callables in the batch path see the same host arrays as in the loop: STOI by the one-clip function, per clip
    called = handoff.denoise_files(jm, dli, str(tmp_path / "called"), snr=10, stoi_fn=metrics.stoi, pesq_fn=pesq_fn,
                                   batch_metrics=True)
    assert [c["stoi"] for c in called] == [a["stoi"] for a in loop]
    none = handoff.denoise_files(jm, dli, str(tmp_path / "none"), snr=10, batch_metrics=True, save_individual_results=False)
    assert all(m["stoi"] is None and m["pesq"] is None and m["csig"] is None and isinstance(m["l1"], float) for m in none)
    assert all(list(m) == list(loop[0])[:19] for m in none)


def test_files_without_a_clean_signal_are_untouched_by_the_flag(tmp_path):
    from sos_amd import handoff
    from sos_amd.detector import networks as dnet
    root = str(tmp_path / "ds")
    _make_dataset(root)
    det = dnet.get_network()
    det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
    det = det.cuda().eval()
    jm = _net()
    out1 = str(tmp_path / "m1_out")
    handoff.detect_files(det, os.path.join(root, "dataset.json"), out1, data_root=root)
    pred_json = handoff.create_data_from_prediction(os.path.join(out1, "eval_results.json"), data_root=root)
    dli = handoff.get_data_from_first_model(pred_json, sr=14000, unknown_clean_signal=True)
    off = handoff.denoise_files(jm, dli, str(tmp_path / "off"))
    on = handoff.denoise_files(jm, dli, str(tmp_path / "on"), batch_metrics=True, stoi_fn=True)
    assert len(off) == len(on) == 2
    for a, b in zip(off, on):
        assert list(a) == list(b) == ["id", "path", "mixed_audio_path", "bitstream", "sr", "snr"] + list(WAVES)
        assert all(a[k] == b[k] for k in list(a)[:6])
        _same_files(a, b, WAVES)
    j = [json.loads(_read(os.path.join(str(tmp_path / d), "eval_results.json"))) for d in ("off", "on")]
    assert list(j[0]) == list(j[1]) and "denoise_statistics" not in j[1]
    for fa, fb in zip(j[0]["files"], j[1]["files"]):
        assert {k: v for k, v in fa.items() if k not in WAVES} == {k: v for k, v in fb.items() if k not in WAVES}
