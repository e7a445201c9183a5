"""The silent-interval labeller on the MI355X (sos_amd.labels, csrc/silence_label.hip) against the float64 restatement
tests/silence_reference.py.  Bits must be equal on every frame: tests/test_silence_reference.py asserts, for the same generators
and seeds, that no frame of these inputs lies within the summation-order band around its threshold.  Energies within 2 m u
relative (m = the clip's longest frame in samples, u = 2^-53): both sums are within (m - 1) u of the exact one.  Parity with the
reference's own labeller is unpinned."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import silence_reference as R

pytestmark = pytest.mark.gpu
GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handoff", "dataset_sounds_of_silence.json")


def _agree(bits, det, want, what):
    assert np.array_equal(bits, want["bits"]), (what, np.flatnonzero(bits != want["bits"])[:8])
    assert bits.dtype == np.uint8 and len(det["energy"]) == want["frames"]
    dev = np.max(np.abs(det["energy"] - want["energy"]) / np.maximum(want["energy"], 1e-300))
    print(f"DEV energy {what} {dev / R.U:.1f} u (bound {2 * want['longest']} u)")
    assert np.all(np.abs(det["energy"] - want["energy"]) <= 2 * want["longest"] * R.U * want["energy"]), what
    assert det["silent_frames"] == want["silent_frames"] and det["silent_runs"] == want["silent_runs"], what
    assert abs(det["max_energy"] - want["max_energy"]) <= 2 * want["longest"] * R.U * want["max_energy"]
    assert abs(det["threshold"] - want["threshold"]) <= (2 * want["longest"] + 2) * R.U * want["threshold"]


@functools.lru_cache(maxsize=None)
def _tile_inputs(sr, fps):
    return [(name, R.plan_samples(plan, sr, fps, seed=len(plan))) for name, plan in R.tile_cases(sr, fps)]


@pytest.mark.parametrize("sr,fps", R.RATES)
def test_plan_clips_around_the_scan_tile(sr, fps):
    from sos_amd import labels
    cases = _tile_inputs(sr, fps)
    xs = [x for _, x in cases]
    sec = R.MIN_FRAMES / fps
    assert R.seconds_to_frames(sec, fps) == R.MIN_FRAMES
    raw, raw_det = labels.silence_bits_batch(xs, sr, fps, min_silence=0.0, min_speech=0.0, return_detail=True)
    got, det = labels.silence_bits_batch(xs, sr, fps, min_silence=sec, min_speech=sec, return_detail=True)
    for (name, x), (_, plan), b0, d0, b, d in zip(cases, R.tile_cases(sr, fps), raw, raw_det, got, det):
        assert np.array_equal(b0, plan), name                              # both passes disabled: the plan itself
        _agree(b0, d0, R.label(x, sr, fps), f"{name} raw")
        _agree(b, d, R.label(x, sr, fps, 40.0, R.MIN_FRAMES, R.MIN_FRAMES), name)


@pytest.mark.parametrize("sr,fps", R.RATES)
def test_shortest_clips_and_a_last_frame_of_one_sample(sr, fps):
    from sos_amd import labels
    ratio = sr / fps
    xs = [np.full(1, 0.25, np.float32), np.full(int(ratio), -0.25, np.float32),
          R.plan_samples(R.plan_from_string("1101"), sr, fps, seed=4, last_frame_samples=1),
          R.plan_samples(R.plan_from_string("1101"), sr, fps, seed=4)]
    got, det = labels.silence_bits_batch(xs, sr, fps, min_silence=0.0, return_detail=True)
    assert [len(b) for b in got] == [1, 1, 4, 4]
    for i, (x, b, d) in enumerate(zip(xs, got, det)):
        _agree(b, d, R.label(x, sr, fps), f"short {i}")
    assert got[0].tolist() == [1] and got[2].tolist() == [1, 1, 0, 1] and det[2]["energy"][3] == np.float64(np.float32(R.LOUD)) ** 2


def test_all_zero_constant_and_minimum_lengths_beyond_the_clip():
    from sos_amd import labels
    sr, fps = 14000, 30.0
    zero = np.zeros(9000, np.float32)
    const = np.where(np.random.default_rng(1).integers(0, 2, size=9000) == 1, 0.2, -0.2).astype(np.float32)
    b, d = labels.silence_bits(zero, sr, fps, return_detail=True)
    assert len(b) == 20 and not b.any() and d["silent_runs"] == 1 and d["silent_frames"] == 20 and d["max_energy"] == 0.0
    b, d = labels.silence_bits(const, sr, fps, return_detail=True)
    assert b.all() and d["silent_runs"] == 0 and d["silent_frames"] == 0
    # min_silence longer than the clip: every quiet run turns non-silent
    name, plan = [c for c in R.tile_cases(sr, fps) if c[0] == "random513"][0]
    x = R.plan_samples(plan, sr, fps, seed=513)
    assert (plan == 0).any()
    b, d = labels.silence_bits(x, sr, fps, min_silence=60.0, return_detail=True)
    assert b.all() and d["silent_frames"] == 0
    _agree(b, d, R.label_seconds(x, sr, fps, min_silence=60.0), "min_silence 60 s")
    # min_speech of 10 000 frames on 513: every loud run between quiet ones turns quiet, those at the ends stay
    b, d = labels.silence_bits(x, sr, fps, min_silence=0.0, min_speech=10000 / fps, return_detail=True)
    want = R.label(x, sr, fps, 40.0, 1, 10000)
    _agree(b, d, want, "min_speech 10000 frames")
    inner = np.flatnonzero(plan == 0)
    assert not b[inner[0]:inner[-1] + 1].any() and want["silent_runs"] == 1


@pytest.mark.parametrize("threshold_db", [20.0, 40.0])
def test_speechlike_clips_at_mixed_rates(threshold_db):
    from sos_amd import labels
    cases = R.speech_cases()
    xs, srs, fpss = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    got, det = labels.silence_bits_batch(xs, srs, fpss, threshold_db, return_detail=True)
    for i, ((x, sr, fps), b, d) in enumerate(zip(cases, got, det)):
        _agree(b, d, R.label_seconds(x, sr, fps, threshold_db), f"speech {i} at {threshold_db} dB")


def test_a_clip_gets_the_same_bits_alone_in_any_batch_and_from_gpu_tensors():
    from sos_amd import labels
    cases = R.batch_cases()
    xs, srs, fpss = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    got, det = labels.silence_bits_batch(xs, srs, fpss, return_detail=True)
    rev, rdet = labels.silence_bits_batch(xs[::-1], srs[::-1], fpss[::-1], return_detail=True)
    ten, tdet = labels.silence_bits_batch([torch.from_numpy(x).cuda() for x in xs], srs, fpss, return_detail=True)
    for i, (x, sr, fps) in enumerate(cases):
        one, odet = labels.silence_bits(x, sr, fps, return_detail=True)
        _agree(one, odet, R.label_seconds(x, sr, fps), f"batch clip {i}")
        for b, d in ((got[i], det[i]), (rev[11 - i], rdet[11 - i]), (ten[i], tdet[i])):
            assert np.array_equal(b, one) and np.array_equal(d["energy"], odet["energy"])         # bit-identical f64
            assert d["threshold"] == odet["threshold"] and d["silent_runs"] == odet["silent_runs"]


def test_chunks_of_a_large_batch_and_bad_inputs(monkeypatch):
    from sos_amd import labels, metrics
    cases = R.batch_cases()[:7]
    xs, srs, fpss = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    want = labels.silence_bits_batch(xs, srs, fpss)
    monkeypatch.setattr("sos_amd.ragged.MAX_CLIPS", 3)
    got = labels.silence_bits_batch(xs, srs, fpss)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert labels.silence_bits_batch([], 14000) == []
    with pytest.raises(ValueError, match="clip 1"):
        labels.silence_bits_batch([xs[0], xs[0][:0]], 14000)
    for sr, fps in ((0, 30.0), (14000, 0.0), (-1, 30.0), (30, 30.0), (20, 30.0)):
        with pytest.raises(ValueError, match="clip 0"):
            labels.silence_bits(xs[0], sr, fps)
    with pytest.raises(ValueError):
        labels.silence_bits_batch(xs, srs[:3], 30.0)
    with pytest.raises(RuntimeError):
        labels.silence_bits(torch.from_numpy(xs[0]), 14000)


def test_the_device_result_goes_straight_into_ragged_stage():
    from sos_amd import labels, tools
    cases = R.batch_cases()[3:9]
    xs, srs, fpss = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    lb = labels.silence_bits_batch_device(xs, srs, fpss)
    stride = max(len(x) for x in xs) + 5
    wave, masked, mask = tools.ragged_stage(lb.flat, lb.table, stride, lb.bits, lb.ratios)
    host_bits = labels.silence_bits_batch(xs, srs, fpss)
    assert np.array_equal(lb.bits.cpu().numpy(), np.concatenate(host_bits))
    assert np.array_equal(lb.ratios, np.asarray(srs) / np.asarray(fpss))
    again = torch.from_numpy(np.concatenate(host_bits)).cuda()
    wave2, masked2, mask2 = tools.ragged_stage(lb.flat, lb.table, stride, again, lb.ratios)
    n_all = sum(len(x) for x in xs)                                          # (flat and the masks end in one unused sentinel sample)
    assert torch.equal(mask[:n_all], mask2[:n_all]) and torch.equal(masked, masked2) and torch.equal(wave, wave2)
    m = mask[:n_all].cpu().numpy()
    assert 0 < m.sum() < n_all                                               # silent samples, and others
    off = 0
    for i, (x, b) in enumerate(zip(xs, host_bits)):
        one = tools.bits_to_mask_batch(torch.from_numpy(b).cuda()[None], srs[i] / fpss[i], len(x))[0].cpu().numpy()
        assert np.array_equal(m[off:off + len(x)], one), i
        off += len(x)


def test_device_entries_that_disagree_with_the_host_get_status_minus_one():
    """The kernels follow the DEVICE table and parameters; a clip that leaves what the host's sized is not labelled, the others
    are.  Clip 1's sample count (then its frame count, then its ratio) is changed on the device after the host's checks."""
    from sos_amd import _lib as L
    from sos_amd import labels
    h = L.lib()
    sr, fps = 14000, 30.0
    xs = [R.plan_samples(R.plan_from_string(p), sr, fps, seed=i) for i, p in enumerate(("1101", "10011", "0111"))]
    want = [R.label(x, sr, fps) for x in xs]
    lens = [len(x) for x in xs]
    tab, par = labels._plan(lens, [sr] * 3, [fps] * 3, 40.0, 0.0, 0.0, 0.0)
    flat = torch.from_numpy(np.concatenate(xs + [np.zeros(1, np.float32)])).cuda()
    need = h.sos_silence_label_workspace_bytes(tab.ctypes.data, 3)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ftot = int(tab[:, 3].sum())
    for what, col, value in (("samples", 1, lens[1] + 1), ("frames", 3, 6), ("frame offset", 2, ftot - 4), ("ratio", None, 1.0)):
        d_tab, d_par = torch.from_numpy(tab).cuda(), torch.from_numpy(par).cuda()
        if col is None:
            d_par[1, 0] = value
        else:
            d_tab[1, col] = value
        bits = torch.full((ftot,), 7, dtype=torch.uint8, device="cuda")
        energy = torch.full((ftot,), -1.0, dtype=torch.float64, device="cuda")
        out = torch.zeros((3, 6), dtype=torch.float64, device="cuda")
        assert h.sos_silence_label_batch(L.ptr(flat), L.ptr(d_tab), tab.ctypes.data, 3, L.ptr(d_par), par.ctypes.data, L.ptr(ws),
                                         need, L.ptr(bits), L.ptr(energy), L.ptr(out), L.stream_ptr()) == 0, what
        o, b, e = out.cpu().numpy(), bits.cpu().numpy(), energy.cpu().numpy()
        assert o[1, 5] == -1 and o[1, 4] == -1 and o[0, 5] == 0 and o[2, 5] == 0, (what, o)
        assert np.all(b[4:9] == 7) and np.all(e[4:9] == -1.0), what          # nothing written for the refused clip
        for i, (f0, F) in ((0, (0, 4)), (2, (9, 4))):
            assert np.array_equal(b[f0:f0 + F], want[i]["bits"]) and o[i, 4] == F and o[i, 2] == want[i]["silent_frames"], (what, i)
    with pytest.raises(RuntimeError, match="clip 1"):
        rows = o.copy()
        labels._check_summary(rows, tab)


def test_label_files_writes_the_data_set_json_the_loader_reads(tmp_path):
    from sos_amd import audio_io, labels
    from sos_amd.dataset import PHASE_TESTING, get_dataloader
    with open(GOLDEN_JSON) as fp:
        golden = json.load(fp)
    rng = np.random.default_rng(5)
    a = R.speechlike(41, 3.1, 14000)
    b = R.speechlike(42, 2.6, 44100)
    c = R.speechlike(43, 2.2, 14000)
    paths = [str(tmp_path / "spk1" / "a.wav"), str(tmp_path / "spk2" / "b.wav"), str(tmp_path / "spk2" / "c.wav")]
    os.makedirs(tmp_path / "spk1")
    os.makedirs(tmp_path / "spk2")
    audio_io.write_wav(paths[0], a, 14000)
    audio_io.write_wav(paths[1], np.stack([b, 0.5 * b]), 44100)              # stereo
    audio_io.write_wav(paths[2], c, 14000)
    noise = str(tmp_path / "noise.wav")
    audio_io.write_wav(noise, (0.1 * rng.standard_normal(3 * 14000)).astype(np.float32), 14000)
    out_json = str(tmp_path / "dataset.json")
    ds = labels.label_files(paths, output_json=out_json)
    small = labels.label_files(paths, max_bytes=4 * 14000)                   # every file a group of its own
    with open(out_json) as fp:
        back = json.load(fp)
    assert json.loads(json.dumps(ds)) == back == json.loads(json.dumps(small))
    assert list(back.keys()) == list(golden.keys()) and back["num_videos"] == 3 and back["dataset_path"] == str(tmp_path)
    for f, path in zip(back["files"], paths):
        assert list(f.keys()) == list(golden["files"][0].keys())
        y, sr = audio_io.load(path, sr=None)
        assert f["path"] == f["audio_path"] == path and f["audio_sample_rate"] == sr and f["audio_samples"] == len(y)
        assert f["framerate"] == 30 and f["duration"] == f["clip_end_time"] == round(len(y) / sr, 2)
        assert f["frames_path"] is None and f["flows_path"] is None and f["clip_start_time"] == f["face_x"] == f["face_y"] == 0
        bits, det = labels.silence_bits(y, sr, return_detail=True)
        assert len(f["bit_stream"]) == f["num_frames"] == len(bits) == R.frame_count(len(y), sr, 30.0)
        assert f["bit_stream"] == "".join(str(int(v)) for v in bits) and set(f["bit_stream"]) == {"0", "1"}
        assert f["silence_total_ratio"] == det["silent_frames"] / len(bits)
        assert abs(f["avg_silenceInterval_silcenceTotal_ratio"] - 1.0 / det["silent_runs"]) < 1e-15
    loader = get_dataloader(PHASE_TESTING, batch_size=16, dataset_json=out_json, noise_files=[noise], model="detector", num_workers=0)
    batches = list(loader)
    assert len(batches) == 1
    label = batches[0]["label"].cpu().numpy()
    windows = [f["bit_stream"][x:x + 60] for f in back["files"] for x in range(0, f["num_frames"] + 1 - 60, 30)]
    assert len(windows) == label.shape[0] >= 3 and label.shape[1] == 60
    for row, w in zip(label, windows):
        assert "".join(str(int(v)) for v in row) == w
