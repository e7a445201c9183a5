"""STOI / extended STOI on the MI355X (sos_amd.metrics.stoi / stoi_batch, csrc/stoi.hip) against the float64
restatement tests/stoi_reference.py: scores within 5e-5, kept-frame counts exact, ragged batches scored clip by clip with
the same bits as single clips in any order, pystoi's edge cases, and the hand-off's stoi_fn hook."""
import json
import os
import warnings

import numpy as np
import pytest
import scipy.io.wavfile
import torch

import stoi_reference as R
from oracle import nets as onet
from oracle import wave_io as owio

pytestmark = pytest.mark.gpu
TOL = 5e-5


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("fs", [8000, 10000, 14000, 16000])
def test_score_and_kept_frames_match_the_oracle(fs, extended):
    from sos_amd import metrics
    x, y = R.closed_form_pair(21, int(3.3 * fs), fs, 0.05)
    want = R.analyse(x, y, fs, extended)
    assert want["margin_db"] > 1e-3 and want["stft_frames"] >= R.N
    got, kept = metrics.stoi_batch([x], [y], fs, extended, return_frames=True)
    assert kept == [want["kept_frames"]]
    assert abs(got[0] - want["score"]) < TOL, (got[0], want["score"])
    assert metrics.stoi(x, y, fs, extended) == got[0]


@pytest.mark.parametrize("extended", [False, True])
def test_ragged_batch_matches_the_oracle_and_single_clips_bit_for_bit(extended):
    from sos_amd import metrics
    rng = np.random.default_rng(31)
    fs = 16000
    lens = rng.integers(1 * fs, 10 * fs + 1, size=64)
    noise = rng.uniform(0.002, 0.5, size=64)
    pairs = [R.closed_form_pair(100 + 2 * i, int(n), fs, float(s)) for i, (n, s) in enumerate(zip(lens, noise))]
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    got, kept = metrics.stoi_batch(xs, ys, fs, extended, return_frames=True)
    for i, (x, y) in enumerate(pairs):
        want = R.analyse(x, y, fs, extended)
        assert want["margin_db"] > 1e-3
        assert kept[i] == want["kept_frames"], i
        assert abs(got[i] - want["score"]) < TOL, (i, got[i], want["score"])
        assert metrics.stoi(x, y, fs, extended) == got[i], i          # alone: the same bits
    perm = rng.permutation(64)
    shuffled = metrics.stoi_batch([xs[i] for i in perm], [ys[i] for i in perm], fs, extended)
    assert [shuffled[j] for j in np.argsort(perm)] == got


def test_too_short_clips_return_1e5_and_warn():
    from sos_amd import metrics
    fs = 10000
    clips = [R.closed_form_pair(41, n, fs, 0.1) for n in (0, 100, 256, 4096, 30000)]
    with pytest.warns(RuntimeWarning, match="Not enough STFT frames"):
        got, kept = metrics.stoi_batch([c[0] for c in clips], [c[1] for c in clips], fs, return_frames=True)
    for (x, y), g, k in zip(clips[:4], got, kept):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            want = R.analyse(x, y, fs)
        assert g == 1e-5 and k == want["kept_frames"]
    assert abs(got[4] - R.stoi(*clips[4], fs)) < TOL
    with pytest.warns(RuntimeWarning):
        assert metrics.stoi(clips[1][0], clips[1][1], fs, extended=True) == 1e-5


@pytest.mark.parametrize("extended", [False, True])
def test_clip_silent_but_for_a_burst_is_scored_on_the_burst(extended):
    from sos_amd import metrics
    fs = 16000
    x, y = R.closed_form_pair(51, 5 * fs, fs, 0.05)
    x[: 2 * fs] = 0.0                                   # silent apart from 1.5 s (about 115 frames at 10 kHz)
    x[int(3.5 * fs):] = 0.0
    want = R.analyse(x, y, fs, extended)
    assert want["margin_db"] > 1e-3 and R.N <= want["stft_frames"] < 130
    got, kept = metrics.stoi_batch([x], [y], fs, extended, return_frames=True)
    assert kept == [want["kept_frames"]] and abs(got[0] - want["score"]) < TOL


@pytest.mark.parametrize("extended", [False, True])
def test_chunks_of_a_large_batch_give_the_same_bits(extended, monkeypatch):
    """More clips than one launch sequence takes (65535) go in chunks; exercised with 7 clips in chunks of 3.  Every clip keeps
    at least 30 frames (tests/stoi_reference.py: 42, 42, 42, 43, 49, 54 and 60), so every one is really scored."""
    from sos_amd import metrics
    fs = 10000
    pairs = [R.closed_form_pair(300 + 2 * i, 8000 + 700 * i, fs, 0.1) for i in range(7)]
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    want, want_kept = metrics.stoi_batch(xs, ys, fs, extended, return_frames=True)
    assert all(k >= 30 for k in want_kept), want_kept
    monkeypatch.setattr("sos_amd.ragged.MAX_CLIPS", 3)
    got, kept = metrics.stoi_batch(xs, ys, fs, extended, return_frames=True)
    assert got == want and kept == want_kept


def test_device_table_entries_outside_the_hosts_lengths_are_not_followed():
    """The kernels take offsets and lengths from the device table; a clip that leaves the samples the host's lengths sum to gets
    status -1 and is not read.  At 10 kHz (p == q) 9000 and 9001 samples make the same 69 frames, so only the bounds rule
    (csrc/ragged.h) can refuse the clip; at 16 kHz the longer resampled copy refuses it as well.  The overrun by one sample lies
    inside the allocation."""
    import ctypes as C
    from sos_amd import _lib as L
    from sos_amd import metrics
    h = L.lib()
    lens = np.asarray([5000, 9000], dtype=np.int64)
    lp = lens.ctypes.data_as(C.c_void_p)
    buf = torch.zeros(14001, device="cuda")
    tab = torch.tensor([[0, 5000], [5000, 9001]], dtype=torch.int64, device="cuda")         # the second clip overruns
    for p, q in ((1, 1), (5, 8)):
        taps = metrics._stoi_taps(p, q, buf.device) if p != q else None
        need = h.sos_stoi_workspace_bytes(lp, 2, p, q)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
        assert h.sos_stoi_batch(L.ptr(buf), L.ptr(buf), L.ptr(tab[0]), L.ptr(tab[1]), lp, 2, p, q, L.ptr(taps),
                                0 if taps is None else taps.numel(), 0, L.ptr(ws), need, L.ptr(out), L.stream_ptr()) == 0
        o = out.cpu().numpy()
        assert o[0, 2] >= 0 and o[1, 2] == -1, (p, q, o)


def test_bad_inputs_raise():
    from sos_amd import metrics
    x, y = R.closed_form_pair(61, 30000, 10000, 0.1)
    with pytest.raises(ValueError):
        metrics.stoi(x, y[:-1], 10000)
    with pytest.raises(ValueError):
        metrics.stoi_batch([x, x], [y, y[:-5]], 10000)
    with pytest.raises(RuntimeError):
        metrics.stoi(torch.from_numpy(x), torch.from_numpy(y), 10000)


def test_gpu_tensors_give_the_numpy_result():
    from sos_amd import metrics
    x, y = R.closed_form_pair(71, 48000, 16000, 0.1)
    for extended in (False, True):
        a = metrics.stoi(x, y, 16000, extended)
        b = metrics.stoi(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 16000, extended)
        c = metrics.stoi(torch.from_numpy(x.astype(np.float64)).cuda(), torch.from_numpy(y).cuda(), 16000, extended)
        assert a == b == c


def test_denoise_files_reports_stoi_through_the_hook(tmp_path):
    """handoff.denoise_files(..., stoi_fn=metrics.stoi): a finite stoi in (0, 1] in stat.json, avg_stoi equal to it, and
    the oracle's STOI of the written files (resampled to 16 kHz as the hand-off does) within 1e-3.  Set-up copied from
    tests/test_gpu_handoff.py::test_known_clean_signal_path_reports_the_objective_measures."""
    from sos_amd import audio_io, handoff, metrics
    from sos_amd.common import MyConfig
    from sos_amd.denoiser import networks as jnet
    root = tmp_path / "m1"
    (root / "recovered").mkdir(parents=True)
    rng = np.random.default_rng(9)
    n, nfr = 14000 * 2, 60
    t = np.arange(n) / 14000
    clean = (0.3 * np.sin(2 * np.pi * 300 * t) * (0.2 + (np.sin(2 * np.pi * 1.3 * t) > -0.4)) + 0.003 * rng.standard_normal(n)).astype(np.float32)
    noise = (0.05 * rng.standard_normal(n)).astype(np.float32)
    for name, sig in (("c_clean", clean), ("c_full_noise", noise), ("c_mixed", clean + noise)):
        audio_io.write_wav(str(root / "recovered" / (name + ".wav")), sig, 14000)
    bits = "".join("1" if (i // 10) % 3 else "0" for i in range(nfr))
    pd = dict(dataset_path="/a", num_videos=1, data_total_frames=60, data_center_frames=1, sigmoid_threshold=0.5, snr=10,
              files=[dict(path="/a/c.wav", framerate=30, bit_stream="1" * nfr, recovered_prediction=bits,
                          mixed_audio="recovered/c_mixed.wav", clean_audio="recovered/c_clean.wav",
                          full_noise="recovered/c_full_noise.wav")])
    with open(root / "pred_data_snr10.json", "w") as fp:
        json.dump(pd, fp)
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    jm = jm.cuda().eval()
    dli = handoff.get_data_from_first_model(str(root / "pred_data_snr10.json"), sr=14000, unknown_clean_signal=False)
    out = str(tmp_path / "m2")
    stat = handoff.denoise_files(jm, dli, out, snr=10, stoi_fn=metrics.stoi)
    info = stat[0]
    assert isinstance(info["stoi"], float) and np.isfinite(info["stoi"]) and 0 < info["stoi"] <= 1
    _, yw = scipy.io.wavfile.read(info["denoised_output"])
    _, cw = scipy.io.wavfile.read(info["ground_truth_clean_input"])
    y16, c16 = owio.resample(yw, 14000, 16000).astype(np.float32), owio.resample(cw, 14000, 16000).astype(np.float32)
    assert abs(info["stoi"] - R.stoi(c16, y16, 16000)) < 1e-3
    with open(os.path.join(out, "eval_results_snr10.json")) as fp:
        ev = json.load(fp)
    assert ev["denoise_statistics"]["avg_stoi"] == info["stoi"]
