"""The file chain in ragged groups: handoff.detect_files(batch_files=True) and handoff.denoise_first_model against the per-file
functions on the same networks and files, in the bf16x3 parity mode.  Bounds: confidences within 2e-4 (the bound
tests/test_gpu_handoff.py puts on them against the oracle), decisions equal; every WAVE file within 2e-4 of the per-file one's
peak (the ragged-versus-alone bound of tests/test_gpu_pipeline.py in bf16x3); the measures of a file within 1e-9 relative
(METRIC_RTOL, batch versus loop) of metrics.evaluate_metrics recomputed from the WAVE files the batched run itself wrote."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import nets as onet
from test_gpu_handoff import _make_dataset

pytestmark = pytest.mark.gpu
METRIC_RTOL = 1e-9
WAVE_TOL = 2e-4
CONF_TOL = 2e-4
WAVES = ("noisy_input", "noise_intervals", "predicted_full_noise", "denoised_output")
GT_WAVES = ("ground_truth_full_noise", "ground_truth_clean_input")
METRIC_KEYS = ("l1", "stoi", "csig", "cbak", "covl", "pesq", "ssnr_regular", "ssnr_shift", "ssnr_clip", "ssnr_exsi", "overall_snr")


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


def _detector(shift=0.0):
    from sos_amd.detector import networks as dnet
    sd = onet.closed_form_state(onet.detector_spec(), seed=1)
    sd["fc1.2.bias"] = sd["fc1.2.bias"] - shift
    det = dnet.get_network()
    det.load_state_dict(sd)
    return det.cuda().eval()


def _fixture(root, specs=(("c", 2.0, 30, 14000), ("d", 1.3, 25, 14000), ("e", 1.7, 30, 16000), ("f", 0.8, 30, 14000)),
             bad_bit=False):
    """pred_data_snr10.json with clean_audio / full_noise entries like test_gpu_handoff_batch._known_clean_fixture: four files of
    2.0, 1.3, 1.7 and 0.8 s (0.8 s = 71 STFT frames at 14 kHz, just above MIN_FRAMES), `d` at framerate 25, `e` stored at
    16 kHz (its three files are the one resampling group)."""
    from sos_amd import audio_io
    (root / "recovered").mkdir(parents=True)
    rng = np.random.default_rng(9)
    files = []
    for name, secs, fr, rate in specs:
        n, nfr = int(rate * secs), int(round(fr * secs))
        t = np.arange(n) / rate
        clean = (0.3 * np.sin(2 * np.pi * 300 * t) * (0.2 + (np.sin(2 * np.pi * 1.3 * t) > -0.4))
                 + 0.003 * rng.standard_normal(n)).astype(np.float32)
        noise = (0.05 * rng.standard_normal(n)).astype(np.float32)
        for suffix, sig in (("_clean", clean), ("_full_noise", noise), ("_mixed", clean + noise)):
            audio_io.write_wav(str(root / "recovered" / (name + suffix + ".wav")), sig, rate)
        bits = "".join("1" if (i // 10) % 3 else "0" for i in range(nfr))
        gt = "".join("0" if (i // 7) % 4 == 1 else "1" for i in range(nfr))
        if bad_bit:
            bits = bits[:3] + "x" + bits[4:]
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
    """The per-file reference (get_data_from_first_model + denoise_files) and the batched run, each with and without known clean
    signals, computed once in bf16x3 and left unchanged."""
    import sos_amd
    from sos_amd import handoff
    root = tmp_path_factory.mktemp("files_batch")
    path = _fixture(root / "m1")
    jm = _denoiser()
    sos_amd.set_precision("bf16x3")
    try:
        res = dict(json=path, jm=jm, root=root)
        for known in (True, False):
            tag = "known" if known else "unknown"
            dli = handoff.get_data_from_first_model(path, sr=14000, unknown_clean_signal=not known)
            res["loop_" + tag] = handoff.denoise_files(jm, dli, str(root / ("loop_" + tag)), snr=10, stoi_fn=True, pesq_fn=_pesq,
                                                       batch_metrics=True)
            del dli
            res["batch_" + tag] = handoff.denoise_first_model(jm, path, str(root / ("batch_" + tag)), sr=14000, snr=10,
                                                              unknown_clean_signal=not known, stoi_fn=True, pesq_fn=_pesq)
    finally:
        sos_amd.set_precision("bf16")
    return res


def _wave(path):
    from sos_amd import audio_io
    arr, kind, rate = audio_io.read_wave(path)
    return arr, kind, rate


def _compare_stats(loop, batch, names, label):
    assert len(loop) == len(batch) == 4
    assert [b["id"] for b in batch] == ["c", "d", "e", "f"]                    # the JSON's file order
    for a, b in zip(loop, batch):
        assert list(a) == list(b)
        for k in a:
            if k in names:
                assert os.path.basename(a[k]) == os.path.basename(b[k]) == k + ".wav"
                assert os.path.basename(os.path.dirname(a[k])) == os.path.basename(os.path.dirname(b[k])) == a["id"]
                assert os.path.basename(os.path.dirname(os.path.dirname(b[k]))) == "snr10"
                (wa, ka, ra), (wb, kb, rb) = _wave(a[k]), _wave(b[k])
                assert (ka, ra, wa.shape, wa.dtype) == (kb, rb, wb.shape, wb.dtype), (a["id"], k)
                err = float(np.abs(wa - wb).max() / np.abs(wa).max())
                print(label, a["id"], k, "samples", wa.shape[0], "max |diff| / peak %.3e" % err)
                assert err < WAVE_TOL, (a["id"], k, err)
            elif k in METRIC_KEYS:
                assert type(a[k]) is type(b[k]), (k, type(a[k]), type(b[k]))
            else:
                assert a[k] == b[k] and type(a[k]) is type(b[k]), k
        with open(os.path.join(os.path.dirname(b["denoised_output"]), "stat.json")) as fp:
            assert json.load(fp) == json.loads(json.dumps(b))


def test_known_clean_signals_equal_the_per_file_chain(chain):
    from sos_amd import audio_io, metrics
    loop, batch = chain["loop_known"], chain["batch_known"]
    assert list(batch[0]) == ["id", "path", "clean_audio_path", "mixed_audio_path", "full_noise_path", "bitstream", "sr", "snr"] + \
        list(METRIC_KEYS) + list(WAVES) + list(GT_WAVES)
    _compare_stats(loop, batch, WAVES + GT_WAVES, "known")
    # the measures, from the files the batched run wrote: pins the pairing of outputs and clean signals
    for b in batch:
        out, _ = audio_io.load_device(b["denoised_output"], sr=None)
        clean, _ = audio_io.load_device(b["ground_truth_clean_input"], sr=None)
        out16, clean16 = audio_io.resample_device(out, 14000, 16000), audio_io.resample_device(clean, 14000, 16000)
        n = min(out16.numel(), clean16.numel())
        want = metrics.evaluate_metrics(out16[:n], clean16[:n], sr=16000, pesq=2.5, stoi=None)
        for k in METRIC_KEYS:
            print(b["id"], k, b[k], want[k])
            if k == "stoi":
                assert isinstance(b[k], float) and 0 < b[k] < 1
                assert abs(b[k] - metrics.stoi(clean16[:n].cpu().numpy(), out16[:n].cpu().numpy(), 16000)) <= METRIC_RTOL * b[k]
                continue
            assert isinstance(b[k], float) and b[k] is not None
            assert abs(b[k] - want[k]) <= METRIC_RTOL * abs(want[k]), (b["id"], k, b[k], want[k])
        assert b["pesq"] == 2.5
    ev = []
    for d in ("loop_known", "batch_known"):
        with open(os.path.join(str(chain["root"] / d), "eval_results_snr10.json")) as fp:
            ev.append(json.load(fp))
    assert list(ev[0]) == list(ev[1]) and list(ev[1]["denoise_statistics"]) == ["avg_" + k for k in METRIC_KEYS]
    assert [list(f) for f in ev[0]["files"]] == [list(f) for f in ev[1]["files"]]
    assert {k: v for k, v in ev[0].items() if k not in ("files", "denoise_statistics")} == \
        {k: v for k, v in ev[1].items() if k not in ("files", "denoise_statistics")}
    assert ev[1]["files"] == json.loads(json.dumps(batch))


def test_unknown_clean_signals_equal_the_per_file_chain(chain):
    loop, batch = chain["loop_unknown"], chain["batch_unknown"]
    assert list(batch[0]) == ["id", "path", "mixed_audio_path", "bitstream", "sr", "snr"] + list(WAVES)
    _compare_stats(loop, batch, WAVES, "unknown")
    ev = []
    for d in ("loop_unknown", "batch_unknown"):
        with open(os.path.join(str(chain["root"] / d), "eval_results_snr10.json")) as fp:
            ev.append(json.load(fp))
    assert list(ev[0]) == list(ev[1]) and "denoise_statistics" not in ev[1]
    for fa, fb in zip(ev[0]["files"], ev[1]["files"]):
        assert {k: v for k, v in fa.items() if k not in WAVES} == {k: v for k, v in fb.items() if k not in WAVES}


def test_two_groups_give_the_order_and_the_signals_of_one(chain):
    from sos_amd import handoff, pipeline
    lens = [torch.empty(n) for n in (28000, 18200, 20825, 11200)]
    assert [len(g) for g in pipeline._ragged_groups(lens, 2, 65536)] == [2, 2]
    assert [len(g) for g in pipeline._ragged_groups(lens, 64, 65536)] == [4]
    two = handoff.denoise_first_model(chain["jm"], chain["json"], str(chain["root"] / "two"), sr=14000, snr=10,
                                      unknown_clean_signal=False, stoi_fn=True, pesq_fn=_pesq, max_batch=2)
    _compare_stats(chain["loop_known"], two, WAVES + GT_WAVES, "max_batch=2")
    for a, b in zip(chain["batch_known"], two):
        for k in METRIC_KEYS:
            assert type(a[k]) is type(b[k])


def test_short_file_and_invalid_bit_are_refused(tmp_path):
    from sos_amd import handoff
    jm = _denoiser()
    short = _fixture(tmp_path / "short", specs=(("c", 2.0, 30, 14000), ("tiny", 0.5, 30, 14000)))
    with pytest.raises(ValueError, match="tiny_mixed.wav"):
        handoff.denoise_first_model(jm, short, str(tmp_path / "out_short"), sr=14000, snr=10)
    assert not os.path.exists(str(tmp_path / "out_short"))
    bad = _fixture(tmp_path / "bad", specs=(("c", 2.0, 30, 14000),), bad_bit=True)
    with pytest.raises(RuntimeError):
        handoff.denoise_first_model(jm, bad, str(tmp_path / "out_bad"), sr=14000, snr=10)


def test_denoise_ragged_with_bits_and_without():
    """bits= / fps= per clip against pipeline.denoise(bits=) of every clip alone (mask bit for bit, signals within the ragged
    bound); without bits the call is the parent's: bit-identical to _denoise_group driven directly."""
    from sos_amd import pipeline, tools
    from sos_amd.dataset import synth_batch
    det, jm = _detector(), _denoiser()
    base = synth_batch(70, 3)["mixed"]
    waves = [base[0][:14000], np.concatenate([base[1], base[2][:123]]), base[2][:11200]]
    clips = [torch.from_numpy(np.ascontiguousarray(w)).cuda() for w in waves]
    outs = pipeline.denoise_ragged(det, jm, clips)
    part = pipeline._ragged_groups(clips, 256, 65536)
    assert len(part) == 1
    ys, _ = pipeline._denoise_group(det, jm, [clips[i] for i in part[0]], pipeline.SR, pipeline.FPS)
    for k, i in enumerate(part[0]):
        assert torch.equal(outs[i], ys[k])
    fps = [30.0, 25.0, 29.97]
    rng = np.random.default_rng(3)
    bits = [rng.integers(0, 2, int(round(len(w) / 14000 * f))).astype(np.uint8) for w, f in zip(waves, fps)]
    got, extra = pipeline.denoise_ragged(None, jm, clips, fps=fps, bits=bits, return_all=True)
    for c, b, f, o, e in zip(clips, bits, fps, got, extra):
        db = torch.from_numpy(b[None]).cuda()
        r = pipeline.denoise(None, jm, c[None], fps=f, bits=db, return_all=True)
        assert torch.equal(e["mask"], tools.bits_to_mask_batch(db, 14000 / f, c.numel())[0]) and torch.equal(e["mask"], r["mask"][0])
        assert torch.equal(e["bits"], db[0])
        err = float((o - r["out"][0]).abs().max() / r["out"][0].abs().max())
        print("denoise_ragged(bits=) clip of", c.numel(), "samples at fps", f, "rel err %.3e" % err)
        assert o.shape == r["out"][0].shape and err < WAVE_TOL
        assert e["noisy_input"].shape == e["noise_intervals"].shape == e["predicted_full_noise"].shape == o.shape
    with pytest.raises(ValueError):
        pipeline.denoise_ragged(det, jm, clips, fps=fps)                       # one fps per clip needs bits
    with pytest.raises(ValueError):
        pipeline.denoise_ragged(None, jm, [clips[0][:7000]], bits=[bits[0][:15]])          # fewer than MIN_FRAMES frames


def test_detect_files_in_groups_equals_per_file(tmp_path):
    from sos_amd import audio_io, handoff
    root = str(tmp_path / "ds")
    _make_dataset(root)
    n = 11200                                                                  # one more recording: 0.8 s at 14 kHz, mono f32
    t = np.arange(n) / 14000
    sig = (0.3 * (np.sin(2 * np.pi * 2.1 * t) > 0) * np.sin(2 * np.pi * 260 * t) + 0.05 * np.random.default_rng(8).standard_normal(n))
    os.makedirs(os.path.join(root, "rec_c"))
    audio_io.write_wav(os.path.join(root, "rec_c", "rec_c_0000001.wav"), sig.astype(np.float32), 14000)
    with open(os.path.join(root, "dataset.json")) as fp:
        ds = json.load(fp)
    ds["files"].append(dict(ds["files"][1], path="/authors/machine/ds/rec_c/rec_c_0000001.wav", clip_end_time=0.8,
                            audio_path="/authors/machine/ds/rec_c/rec_c_0000001.wav", audio_samples=n, duration=0.8,
                            num_frames=24, bit_stream="1" * 24))
    ds["num_videos"] = 3
    with open(os.path.join(root, "dataset.json"), "w") as fp:
        json.dump(ds, fp)
    dj = os.path.join(root, "dataset.json")
    # centre the logits so that both classes occur (as tests/test_gpu_handoff.py does with the oracle's logits)
    first = handoff.detect_files(_detector(), dj, str(tmp_path / "probe"), data_root=root, save_stat=False)
    conf = np.concatenate([np.asarray(it["confidence"], dtype=np.float64) for it in first["data"]])
    conf = np.clip(conf, 1e-6, 1 - 1e-6)
    det = _detector(shift=float(np.median(np.log(conf / (1 - conf)))))
    loop = handoff.detect_files(det, dj, str(tmp_path / "loop"), data_root=root)
    batch = handoff.detect_files(det, dj, str(tmp_path / "batch"), data_root=root, batch_files=True)
    two = handoff.detect_files(det, dj, str(tmp_path / "two"), data_root=root, batch_files=True, max_batch=2)
    labels = [b for it in loop["data"] for b in it["pred_label"]]
    assert "0" in labels and "1" in labels
    for got, name in ((batch, "batch"), (two, "two")):
        assert list(got) == list(loop)
        assert {k: v for k, v in got.items() if k != "data"} == {k: v for k, v in loop.items() if k != "data"}
        assert got["prediction_statistics"] == loop["prediction_statistics"]
        assert [it["id"] for it in got["data"]] == [it["id"] for it in loop["data"]]          # the sort by mean confidence
        for a, b in zip(loop["data"], got["data"]):
            assert list(a) == list(b)
            for k in a:
                if k != "confidence":
                    assert a[k] == b[k] and type(a[k]) is type(b[k]), (a["id"], k)
            ca, cb = np.asarray(a["confidence"], dtype=np.float64), np.asarray(b["confidence"], dtype=np.float64)
            assert ca.shape == cb.shape and all(isinstance(c, str) for c in b["confidence"])
            print(name, "file", a["id"], "frames", len(ca), "max |confidence diff| %.3e" % float(np.abs(ca - cb).max()))
            assert float(np.abs(ca - cb).max()) < CONF_TOL
        with open(os.path.join(str(tmp_path / name), "eval_results.json")) as fp:
            assert json.load(fp) == json.loads(json.dumps(got))
