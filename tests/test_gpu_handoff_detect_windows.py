"""handoff.detect_files(batch_files=True, window_seconds=...): the detector half of the file chain on recordings of any length,
through pipeline.detect_long.  The data set is built as tests/test_gpu_handoff_files_batch.py builds its own (three recordings of
3.2, 2.5 and 0.8 s, one stored as 44.1 kHz stereo int16), in the bf16x3 parity mode."""
import json
import os

import numpy as np
import pytest
import scipy.io.wavfile
import torch

from oracle import nets as onet

pytestmark = pytest.mark.gpu

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
N_LONG = 3 * CORE + 5 * HOP + 77


@pytest.fixture(autouse=True)
def _parity_mode():
    import sos_amd
    sos_amd.set_precision("bf16x3")
    try:
        yield
    finally:
        sos_amd.set_precision("bf16")


def _detector(shift=0.0):
    from sos_amd.detector import networks as dnet
    sd = onet.closed_form_state(onet.detector_spec(), seed=1)
    sd["fc1.2.bias"] = sd["fc1.2.bias"] - shift
    det = dnet.get_network()
    det.load_state_dict(sd)
    return det.cuda().eval()


def _entry(name, sr0, n, secs, framerate, nfr):
    path = "/authors/machine/ds/%s/%s_0000001.wav" % (name, name)
    return dict(path=path, clip_start_time=0, clip_end_time=secs, face_x=0, face_y=0, framerate=framerate, audio_sample_rate=sr0,
                audio_samples=n, duration=secs, num_frames=nfr, bit_stream="1" * nfr, silence_total_ratio=0,
                avg_silenceInterval_silcenceTotal_ratio=0, frames_path=None, flows_path=None, audio_path=path)


def _signal(rng, n, sr0):
    t = np.arange(n) / sr0
    env = (np.sin(2 * np.pi * 0.7 * t) > -0.2).astype(np.float64)            # speech-like on/off envelope
    return 0.3 * env * np.sin(2 * np.pi * 220 * t * (1 + 0.3 * np.sin(2 * np.pi * 3 * t))) + 0.05 * rng.standard_normal(n)


def _write(root, name, sr0, pcm):
    os.makedirs(os.path.join(root, name), exist_ok=True)
    scipy.io.wavfile.write(os.path.join(root, name, name + "_0000001.wav"), sr0, pcm)


def _short_dataset(root):
    """rec_a 3.2 s at 44.1 kHz stereo int16, rec_b 2.5 s and rec_c 0.8 s at 14 kHz mono f32; rec_c's label is one frame
    shorter than its duration gives."""
    rng = np.random.default_rng(5)
    files = []
    for name, sr0, ch, secs, dtype, nfr in (("rec_a", 44100, 2, 3.2, np.int16, 96), ("rec_b", 14000, 1, 2.5, np.float32, 75),
                                            ("rec_c", 14000, 1, 0.8, np.float32, 23)):
        n = int(sr0 * secs)
        sig = _signal(rng, n, sr0)
        pcm = np.stack([sig, 0.8 * sig + 0.01 * rng.standard_normal(n)], axis=1)[:, :ch]
        pcm = np.clip(pcm * 32768, -32768, 32767).astype(np.int16) if dtype == np.int16 else pcm.astype(np.float32)
        _write(root, name, sr0, pcm if ch > 1 else pcm[:, 0])
        files.append(_entry(name, sr0, n, secs, 30, nfr))
    with open(os.path.join(root, "dataset.json"), "w") as fp:
        json.dump(dict(dataset_path="/authors/machine/ds", num_videos=len(files), files=files), fp)
    return os.path.join(root, "dataset.json")


def _centred(dj, root, tmp_path):
    """A detector whose logits on this data set have the median 0, so that both classes occur."""
    from sos_amd import handoff
    first = handoff.detect_files(_detector(), dj, str(tmp_path / "probe"), data_root=root, save_stat=False, batch_files=True)
    conf = np.clip(np.concatenate([np.asarray(it["confidence"], dtype=np.float64) for it in first["data"]]), 1e-6, 1 - 1e-6)
    return _detector(shift=float(np.median(np.log(conf / (1 - conf)))))


@pytest.mark.parametrize("max_batch", [64, 2])
def test_files_shorter_than_two_cores_give_the_same_json_byte_for_byte(tmp_path, max_batch):
    """Every file is one window: that window is the file, run in the same groups."""
    from sos_amd import handoff
    root = str(tmp_path / "ds")
    dj = _short_dataset(root)
    det = _centred(dj, root, tmp_path)
    kw = dict(data_root=root, batch_files=True, max_batch=max_batch, max_columns=65536)
    plain = handoff.detect_files(det, dj, str(tmp_path / "plain"), **kw)
    wind = handoff.detect_files(det, dj, str(tmp_path / "wind"), window_seconds=2.0, context_seconds=0.5, **kw)     # 2 cores > 3.2 s
    labels = [b for it in plain["data"] for b in it["pred_label"]]
    assert "0" in labels and "1" in labels
    with open(str(tmp_path / "plain" / "eval_results.json"), "rb") as a, open(str(tmp_path / "wind" / "eval_results.json"), "rb") as b:
        assert a.read() == b.read()
    assert json.dumps(plain) == json.dumps(wind)
    assert [len(it["pred_label"]) for it in sorted(wind["data"], key=lambda it: it["id"])] == [96, 75, 23]


def test_a_three_window_file_gets_one_decision_per_label_frame(tmp_path):
    from sos_amd import audio_io, handoff, pipeline, tools
    root = str(tmp_path / "ds")
    rng = np.random.default_rng(6)
    files = []
    for name, n, framerate, nfr in (("rec_l", N_LONG, 25, pipeline.n_video_frames(N_LONG, 14000, 25) - 1), ("rec_s", 150 * HOP + 31, 30, 51)):
        _write(root, name, 14000, _signal(rng, n, 14000).astype(np.float32))
        files.append(_entry(name, 14000, n, n / 14000, framerate, nfr))
    dj = os.path.join(root, "dataset.json")
    with open(dj, "w") as fp:
        json.dump(dict(dataset_path="/authors/machine/ds", num_videos=2, files=files), fp)
    det = _detector()
    seconds = dict(window_seconds=CORE / 14000, context_seconds=CONTEXT / 14000)
    stat = handoff.detect_files(det, dj, str(tmp_path / "out"), data_root=root, batch_files=True, **seconds)
    items = sorted(stat["data"], key=lambda it: it["id"])
    assert [it["id"] for it in items] == [0, 1] and list(stat) == ['data_total_frames', 'data_center_frames', 'sigmoid_threshold', 'snr',
                                                                  'prediction_statistics', 'data']
    for it, f in zip(items, files):
        assert len(it["pred_label"]) == len(it["label"]) == len(it["confidence"]) == f["num_frames"]
    # the confidences are threshold_bits' sigmoid of detect_long's stitched logits of the same recordings
    loaded, _ = audio_io.load_batch_device([os.path.join(root, n, n + "_0000001.wav") for n in ("rec_l", "rec_s")], sr=14000)
    assert [int(x.numel()) for x in loaded] == [N_LONG, 150 * HOP + 31]
    pairs = pipeline.detect_long(det, [x.contiguous() for x in loaded], sr=14000, fps=[25, 30], n_frames=[f["num_frames"] for f in files],
                                 max_batch=64, **seconds)
    assert len(pairs[0][0]) == files[0]["num_frames"] and len(pipeline.window_plan([N_LONG], CORE, CONTEXT)) == 3
    for it, (logits, bits) in zip(items, pairs):
        _, conf = tools.threshold_bits(logits, 0.5)
        assert it["confidence"] == [str(c) for c in conf.cpu().numpy()]
        assert it["pred_label"] == [str(int(b)) for b in bits.cpu().numpy()]
    with open(str(tmp_path / "out" / "eval_results.json")) as fp:
        assert json.load(fp) == json.loads(json.dumps(stat))


def test_window_seconds_without_batch_files_raises(tmp_path):
    from sos_amd import handoff
    root = str(tmp_path / "ds")
    dj = _short_dataset(root)
    with pytest.raises(ValueError, match="batch_files"):
        handoff.detect_files(_detector(), dj, str(tmp_path / "out"), data_root=root, window_seconds=2.0)
    assert not os.path.exists(str(tmp_path / "out"))
