"""The clean-recordings branch of the hand-off with the mixing in ragged batches: handoff.detect_files(batch_mix=True) and
handoff.create_data_from_prediction(batch_files=True) against the per-file forms on the same networks, files and seed, in the
bf16x3 parity mode.  Bounds: confidences within CONF_TOL = 2e-4 and WAVE files within WAVE_TOL = 2e-4 of the per-file file's
peak (the bounds of tests/test_gpu_handoff_files_batch.py).  The ragged mix may differ from the one-workgroup kernel's in the
last bit, so a frame whose per-file confidence lies within CONF_TOL of the threshold may flip legitimately: decisions are
compared on every other frame, and the frames set aside may be at most 5 % of all frames."""
import filecmp
import json
import os
import shutil

import numpy as np
import pytest

from test_gpu_handoff import _make_dataset
from test_gpu_handoff_files_batch import CONF_TOL, WAVE_TOL, _detector

pytestmark = pytest.mark.gpu
DECISION_KEYS = ("pred_label", "match", "confidence")


@pytest.fixture(autouse=True)
def _parity_mode():
    import sos_amd
    sos_amd.set_precision("bf16x3")
    try:
        yield
    finally:
        sos_amd.set_precision("bf16")


def _dataset(root):
    """tests/test_gpu_handoff._make_dataset with labelled silent intervals in the first recording and unlabelled frames ('2')
    around the second (its labelled part starts at frame 2: the noise crop is read from that frame's sample on), and two short
    noise recordings (the first shorter than either recording: its crop is zero-filled)."""
    from sos_amd import audio_io
    _make_dataset(root)
    dj = os.path.join(root, "dataset.json")
    with open(dj) as fp:
        ds = json.load(fp)
    a, b = ds["files"]
    a["bit_stream"] = "".join("0" if (i // 9) % 3 == 1 else "1" for i in range(a["num_frames"]))
    b["bit_stream"] = "".join("0" if (i // 11) % 2 else "1" for i in range(b["num_frames"]))
    with open(os.path.join(root, "dataset_plain.json"), "w") as fp:          # every frame labelled: what
        json.dump(ds, fp)                                                    # create_data_from_prediction takes
    b["bit_stream"] = "22" + b["bit_stream"][2:-3] + "222"
    with open(dj, "w") as fp:
        json.dump(ds, fp)
    rng = np.random.default_rng(21)
    noise = []
    for name, secs in (("noise_short", 1.5), ("noise_long", 4.0)):
        noise.append(os.path.join(root, name + ".wav"))
        audio_io.write_wav(noise[-1], (0.1 * rng.standard_normal(int(14000 * secs))).astype(np.float32), 14000)
    return dj, noise


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """detect_files on the clean-recordings branch per file and with batch_mix=True, computed once and left unchanged; and one
    run over the data set without unlabelled frames for create_data_from_prediction."""
    import sos_amd
    from sos_amd import handoff
    tmp = tmp_path_factory.mktemp("mix_batch")
    root = str(tmp / "ds")
    dj, noise = _dataset(root)
    sos_amd.set_precision("bf16x3")
    try:
        kw = dict(data_root=root, noise_files=noise, snr=3, seed=5, batch_files=True)
        # centre the logits so that both classes occur (as tests/test_gpu_handoff_files_batch.py does)
        first = handoff.detect_files(_detector(), dj, str(tmp / "probe"), save_stat=False, **kw)
        conf = np.concatenate([np.asarray(it["confidence"], dtype=np.float64) for it in first["data"]])
        conf = np.clip(conf, 1e-6, 1 - 1e-6)
        det = _detector(shift=float(np.median(np.log(conf / (1 - conf)))))
        loop = handoff.detect_files(det, dj, str(tmp / "loop"), batch_mix=False, **kw)
        batch = handoff.detect_files(det, dj, str(tmp / "batch"), batch_mix=True, **kw)
        two = handoff.detect_files(det, dj, str(tmp / "two"), batch_mix=True, max_mix_bytes=1, **kw)       # a group per file
        handoff.detect_files(det, os.path.join(root, "dataset_plain.json"), str(tmp / "loop_plain"), **kw)
    finally:
        sos_amd.set_precision("bf16")
    return dict(tmp=tmp, root=root, dj=dj, noise=noise, det=det, loop=loop, batch=batch, two=two)


@pytest.mark.parametrize("name", ["batch", "two"])
def test_detect_files_with_the_mix_in_ragged_batches_equals_per_file(runs, name):
    loop, got, tmp = runs["loop"], runs[name], runs["tmp"]
    assert list(got) == list(loop) == ["data_total_frames", "data_center_frames", "sigmoid_threshold", "snr", "prediction_statistics", "data"]
    assert {k: v for k, v in got.items() if k not in ("data", "prediction_statistics")} == \
        {k: v for k, v in loop.items() if k not in ("data", "prediction_statistics")} and got["snr"] == 3
    by_id = {it["id"]: it for it in got["data"]}
    assert sorted(by_id) == sorted(it["id"] for it in loop["data"]) == [0, 1]
    frames = band = 0
    labels = []
    for a in loop["data"]:
        b = by_id[a["id"]]
        assert list(a) == list(b)
        for k in a:
            if k not in DECISION_KEYS:
                assert a[k] == b[k] and type(a[k]) is type(b[k]), (a["id"], k)
        ca, cb = np.asarray(a["confidence"], dtype=np.float64), np.asarray(b["confidence"], dtype=np.float64)
        assert ca.shape == cb.shape == (len(a["label"]),) and all(isinstance(c, str) for c in b["confidence"])
        near = np.abs(ca - 0.5) <= CONF_TOL
        print(name, "file", a["id"], "frames", len(ca), "max |confidence diff| %.3e" % float(np.abs(ca - cb).max()),
              "frames within CONF_TOL of the threshold", int(near.sum()))
        assert float(np.abs(ca - cb).max()) < CONF_TOL
        pa, pb = np.asarray(a["pred_label"]), np.asarray(b["pred_label"])
        assert pa.shape == pb.shape and np.array_equal(pa[~near], pb[~near])
        frames, band = frames + len(ca), band + int(near.sum())
        labels += a["pred_label"]
        if not near.any():
            assert a["match"] == b["match"]
    assert "0" in labels and "1" in labels
    assert band <= 0.05 * frames, (band, frames)                             # the share set aside, in the per-file run alone
    if band == 0:
        assert got["prediction_statistics"] == loop["prediction_statistics"]
        assert [it["id"] for it in got["data"]] == [it["id"] for it in loop["data"]]         # the sort by mean confidence
    # the noise crops and their bookkeeping: the same draws, byte for byte
    da, db = os.path.join(str(tmp / "loop"), "noise_snr3"), os.path.join(str(tmp / name), "noise_snr3")
    assert sorted(os.listdir(da)) == sorted(os.listdir(db)) == ["rec_a_0000001_noise.wav", "rec_b_0000001_noise.wav", "snr3.json"]
    for fn in os.listdir(da):
        assert filecmp.cmp(os.path.join(da, fn), os.path.join(db, fn), shallow=False), fn
    with open(os.path.join(str(tmp / name), "eval_results_snr3.json")) as fp:
        assert json.load(fp) == json.loads(json.dumps(got))


def _wave(path):
    from sos_amd import audio_io
    return audio_io.read_wave(path)


@pytest.mark.parametrize("clean_audio", [True, False], ids=["clean-recordings", "recordings-only"])
def test_create_data_from_prediction_in_batches_equals_per_file(runs, clean_audio):
    from sos_amd import handoff
    tmp = runs["tmp"]
    tag = "clean" if clean_audio else "plain"
    dirs = [str(tmp / ("pred_loop_" + tag)), str(tmp / ("pred_batch_" + tag))]
    out = []
    for d, batch_files in zip(dirs, (False, True)):
        shutil.copytree(str(tmp / "loop_plain"), d)                          # eval_results_snr3.json and noise_snr3/ of one run
        out.append(handoff.create_data_from_prediction(os.path.join(d, "eval_results_snr3.json"), noise_snr=3, data_root=runs["root"],
                                                       clean_audio=clean_audio, batch_files=batch_files))
    assert [os.path.basename(p) for p in out] == ["pred_data_snr3.json"] * 2
    with open(out[0], "rb") as fa, open(out[1], "rb") as fb:
        ra, rb = fa.read(), fb.read()
    assert ra.replace(dirs[0].encode(), b"@") == rb.replace(dirs[1].encode(), b"@")          # the same bytes but for the directory
    pa, pb = json.loads(ra), json.loads(rb)
    assert list(pa) == list(pb) and len(pa["files"]) == len(pb["files"]) == 2
    keys = ("mixed_audio", "clean_audio", "full_noise") if clean_audio else ("mixed_audio",)
    for fa, fb in zip(pa["files"], pb["files"]):
        assert list(fa) == list(fb)
        assert ("audio_path" in fb) == clean_audio
        for k in keys:
            assert fa[k] == fb[k] and fb[k].startswith("recovered_snr3/")
            (wa, ka, ra_), (wb, kb, rb_) = _wave(os.path.join(dirs[0], fa[k])), _wave(os.path.join(dirs[1], fb[k]))
            assert (ka, ra_, wa.shape, wa.dtype) == (kb, rb_, wb.shape, wb.dtype), (fa["path"], k)
            err = float(np.abs(wa - wb).max() / np.abs(wa).max())
            print(tag, os.path.basename(fa["path"]), k, "samples", wa.shape[0], "max |diff| / peak %.3e" % err)
            assert err < WAVE_TOL, (fa["path"], k, err)


def test_batch_mix_needs_batch_files_and_noise_files(runs, tmp_path):
    from sos_amd import handoff
    det, dj, root, noise = runs["det"], runs["dj"], runs["root"], runs["noise"]
    with pytest.raises(ValueError, match="batch_mix"):
        handoff.detect_files(det, dj, str(tmp_path / "a"), data_root=root, noise_files=noise, snr=3, batch_mix=True)
    with pytest.raises(ValueError, match="batch_mix"):
        handoff.detect_files(det, dj, str(tmp_path / "b"), data_root=root, batch_files=True, batch_mix=True)
    assert not os.path.exists(str(tmp_path / "a")) and not os.path.exists(str(tmp_path / "b"))
