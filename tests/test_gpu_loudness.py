"""csrc/loudness.hip on the device: sos_loudness_batch_f64 and sos_loudness_gain_batch_f32 through metrics.loudness_batch /
loudness and audio_io.loudness_gain_batch_device, against tests/loudness_reference.py (itself held against the standard's table
and the EBU Tech 3341 readings in tests/test_loudness_reference.py).
Bounds.  Block counts and flags: equality.  Peaks: equality of bits (a maximum of float32 magnitudes).  L: 1e-6 LU -- the inputs
are exact in double and every operation is double on both sides, so only the order of rounding differs (a chunked scan of the
recurrence against the sequential filter differs by about 1e-14 relative; 1e-6 LU is 2.3e-7 relative in energy).  So that a
difference of that size cannot flip a gate, the test first asserts ON THE REFERENCE that no block of any file lies within 1e-6 LU
of either of its gates.  Gains: 2^-22 relative (two float64 pow calls and one rounding to float32); scaled planes: the bits of
x * g_device, one float32 multiply.
Shapes: ONE ragged call of 24 files at 8000 (h = 800), 11025 (h = 1103, the rounding) and 44100 Hz with 1, 2, 3 and 6 channels;
per rate 4h - 1 (no block), 4h, 5h - 1, 5h and about 3 s (no multiple of h or of a chunk); an all-zero file, one that reads
zeros past its plane, one that is cropped; segments 25 LU apart, a segment below -70 LUFS, a DC offset; planes back to back in
one buffer, so most start off 16 bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import loudness_reference as LR

pytestmark = pytest.mark.gpu
BOUND_LU = 1e-6
SENTINEL = 777.0
SURROUND = [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]


def _noise(rng, ch, n, amp):
    return (amp * rng.standard_normal((ch, n))).astype(np.float32)


def _steps(rng, ch, lengths, amps):
    return np.concatenate([_noise(rng, ch, n, a) for n, a in zip(lengths, amps)], axis=1)


@pytest.fixture(scope="module")
def batch():
    """dict(files=[dict(name, x (channels, avail) float32, sr, frames, weights, ref)], ..): the reference computed once."""
    rng = np.random.default_rng(20261020)
    files = []

    def add(name, x, sr, frames=None, weights=None):
        files.append(dict(name=name, x=np.ascontiguousarray(x, dtype=np.float32), sr=sr, frames=x.shape[1] if frames is None else frames,
                          weights=weights))

    for k, sr in enumerate((8000, 11025, 44100)):
        h = LR.hop(sr)
        for j, n in enumerate((4 * h - 1, 4 * h, 5 * h - 1, 5 * h, 3 * sr + 17 + k)):
            add("%d/%d" % (sr, n), _noise(rng, 1 + (j + k) % 3, n, 0.1), sr)
    add("zero", np.zeros((2, 22050), np.float32), 11025)
    add("zero-filled", _noise(rng, 2, 20000, 0.05), 8000, frames=20000 + 2 * 800 + 37)
    add("cropped", _noise(rng, 1, 30000, 0.2), 11025, frames=30000 - 1434)
    add("25 LU apart", _steps(rng, 2, (66150, 66150 + 13), (0.2, 0.2 * 10.0 ** (-25.0 / 20.0))), 44100)
    add("below -70", _steps(rng, 1, (12000, 12000 + 5), (0.1, 2e-5)), 8000)
    add("dc", _noise(rng, 1, 3 * 44100 + 7, 0.05) + np.float32(0.5), 44100)
    add("5.1", _noise(rng, 6, 24000 + 3, 0.1) * np.asarray([1, 0.5, 0.7, 3.0, 0.4, 0.6], np.float32)[:, None], 8000, weights=SURROUND)
    add("loud spike", np.concatenate([_noise(rng, 1, 16000, 0.002), np.full((1, 1), 0.9, np.float32), _noise(rng, 1, 16000, 0.002)], axis=1), 8000)
    add("fs sine", LR.sine(997.0, 44100, [(0.0, 1.0)]), 44100)
    for f in files:
        f["ref"] = LR.measure(f["x"], f["sr"], f["weights"], f["frames"])
    return files


def _device_planes(files, lead=0):
    """The planes back to back in one buffer, `lead` sentinel floats before and 64 after: (flat, views)."""
    flat = np.concatenate([np.full(lead, SENTINEL, np.float32)] + [f["x"].reshape(-1) for f in files] + [np.full(64, SENTINEL, np.float32)])
    dev = torch.from_numpy(flat).cuda()
    views, at = [], lead
    for f in files:
        views.append(dev[at:at + f["x"].size].view(f["x"].shape))
        at += f["x"].size
    return dev, views


def _measure(files, views, **kw):
    from sos_amd import metrics
    return metrics.loudness_batch(views, [f["sr"] for f in files], [f["weights"] for f in files], [f["frames"] for f in files], **kw)


def _worst(files, rows):
    """Largest |L - L_ref| over the files with a finite reference, after the exact comparisons."""
    worst = 0.0
    for f, (lufs, peak, n_rel, n_abs) in zip(files, rows):
        ref = f["ref"]
        assert (n_rel, n_abs) == (ref["blocks"], ref["blocks_abs"]), (f["name"], n_rel, n_abs, ref)
        assert np.float64(peak).tobytes() == np.float64(ref["peak"]).tobytes(), (f["name"], peak, ref["peak"])
        if np.isfinite(ref["lufs"]):
            worst = max(worst, abs(lufs - ref["lufs"]))
        else:
            assert lufs == ref["lufs"], (f["name"], lufs)
    return worst


def test_the_reference_of_the_batch_is_clear_of_its_gates(batch):
    """Asserted before the device is looked at: every file that has a block and is not silent has one passing block, the two gates
    each drop blocks somewhere, and no block lies within the bound of a gate."""
    for f in batch:
        ref, n = f["ref"], f["frames"]
        assert ref["margin"] > BOUND_LU, (f["name"], ref["margin"])
        if n >= 4 * LR.hop(f["sr"]) and f["name"] != "zero":
            assert ref["blocks"] >= 1, f["name"]
        else:
            assert ref["lufs"] == -np.inf and ref["blocks"] == 0
    by = {f["name"]: f["ref"] for f in batch}
    total = lambda f: (f["frames"] - 4 * LR.hop(f["sr"])) // LR.hop(f["sr"]) + 1                   # noqa: E731
    assert 0 < by["25 LU apart"]["blocks"] < by["25 LU apart"]["blocks_abs"] == total(next(f for f in batch if f["name"] == "25 LU apart"))
    assert 0 < by["below -70"]["blocks_abs"] < total(next(f for f in batch if f["name"] == "below -70"))
    assert abs(by["fs sine"]["lufs"] + 3.01) < 0.02


def test_one_ragged_call_is_the_reference(batch):
    _, views = _device_planes(batch)
    assert sum(v.storage_offset() % 4 != 0 for v in views) >= 10                      # planes off 16 bytes are among them
    got = _measure(batch, views)
    assert set(got) == {"lufs", "peak", "blocks", "blocks_abs", "rows"}
    for key, dtype in (("lufs", torch.float64), ("peak", torch.float64), ("blocks", torch.int64), ("blocks_abs", torch.int64)):
        assert got[key].is_cuda and got[key].dtype == dtype and got[key].shape == (len(batch),)
    rows = got["rows"].cpu().numpy()
    assert np.array_equal(got["lufs"].cpu().numpy(), rows[:, 0]) and got["blocks"].cpu().tolist() == rows[:, 2].tolist()
    worst = _worst(batch, rows)
    print("largest |L - L_ref| over %d files: %.3e LU (bound %.0e)" % (len(batch), worst, BOUND_LU))
    assert worst <= BOUND_LU
    assert torch.equal(_measure(batch, views)["rows"], got["rows"])                   # fixed order of every sum: equal bits


@pytest.mark.parametrize("split", [1, 3, 64])
def test_the_chunk_length_moves_nothing_but_rounding(batch, split):
    """3 divides neither 800 nor 1103 (chunks of two lengths in a hop); 1 is a hop per thread; 64 is the finest."""
    _, views = _device_planes(batch)
    rows = _measure(batch, views, split=split)["rows"].cpu().numpy()
    worst = _worst(batch, rows)
    base = _measure(batch, views)["rows"].cpu().numpy()
    finite = np.isfinite(base[:, 0])
    between = float(np.max(np.abs(rows[finite, 0] - base[finite, 0])))
    print("split %d: largest |L - L_ref| %.3e LU, against split 8 %.3e LU" % (split, worst, between))
    assert worst <= BOUND_LU and between <= BOUND_LU


def test_files_apart_and_one_clip(batch):
    """Planes that do not lie back to back, and metrics.loudness on a 1-D and a 2-D clip."""
    from sos_amd import metrics
    some = [batch[4], batch[-4], batch[9]]
    views = [torch.from_numpy(f["x"]).cuda() for f in some]
    assert _worst(some, _measure(some, views)["rows"].cpu().numpy()) <= BOUND_LU
    sine = next(f for f in batch if f["name"] == "fs sine")
    one = metrics.loudness(sine["x"][0], 44100)
    assert abs(one["lufs"] - sine["ref"]["lufs"]) <= BOUND_LU and abs(one["lufs"] + 3.01) < 0.02 and one["peak"] == sine["ref"]["peak"]
    surround = next(f for f in batch if f["name"] == "5.1")
    six = metrics.loudness(torch.from_numpy(surround["x"]).cuda(), 8000, channel_weights=SURROUND)
    assert abs(six["lufs"] - surround["ref"]["lufs"]) <= BOUND_LU and six["blocks"] == surround["ref"]["blocks"]
    plain = LR.measure(surround["x"], 8000)["lufs"]
    assert abs(plain - surround["ref"]["lufs"]) > 1.0                                 # the loud LFE channel counts 0
    assert abs(metrics.loudness(surround["x"], 8000)["lufs"] - plain) <= BOUND_LU


# ------------------------------------------------------------------------------------------------ the gain
def _gain_case(batch, targets):
    """Measure and scale the batch between sentinels; -> (planes before, buffer after, gains, limited, views, lead)."""
    from sos_amd import audio_io
    lead = 61                                                                          # an odd start: no plane is aligned by luck
    dev, views = _device_planes(batch, lead)
    before = dev.cpu().numpy().copy()
    stats = _measure(batch, views)
    target = torch.from_numpy(np.asarray(targets, np.float64)).cuda() if np.ndim(targets) else targets
    gains, limited = audio_io.loudness_gain_batch_device(views, stats, target, -1.0, frames=[f["frames"] for f in batch])
    assert gains.dtype == torch.float32 and limited.dtype == torch.bool and gains.shape == limited.shape == (len(batch),)
    return before, dev.cpu().numpy(), gains.cpu().numpy(), limited.cpu().numpy(), lead


@pytest.mark.parametrize("per_file", [False, True], ids=["one target", "a target per file"])
def test_gain_scales_the_frames_of_every_file_and_nothing_else(batch, per_file):
    targets = [-20.0 - 0.5 * (i % 7) for i in range(len(batch))] if per_file else -20.0
    before, after, gains, limited, lead = _gain_case(batch, targets)
    assert np.all(after[:lead] == SENTINEL) and np.all(after[-64:] == SENTINEL), "the gain wrote outside the planes"
    at, worst = lead, 0.0
    for i, f in enumerate(batch):
        ref = f["ref"]
        g_ref, lim_ref = LR.gain(ref["lufs"], ref["peak"], targets[i] if per_file else targets, -1.0)
        assert bool(limited[i]) == lim_ref, f["name"]
        worst = max(worst, abs(float(gains[i]) / float(g_ref) - 1.0))
        x = before[at:at + f["x"].size].reshape(f["x"].shape)
        want = LR.apply_gain(x, gains[i], f["frames"])                                # past the frames: the value it had
        got = after[at:at + f["x"].size].reshape(f["x"].shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f["name"]
        at += f["x"].size
    print("largest relative difference of a gain: %.3e (bound 2^-22 = %.3e)" % (worst, 2.0 ** -22))
    assert worst <= 2.0 ** -22
    by = {f["name"]: i for i, f in enumerate(batch)}
    assert limited[by["loud spike"]] and abs(gains[by["loud spike"]] * 0.9 - 10.0 ** (-1.0 / 20.0)) < 1e-6      # the ceiling binds
    assert gains[by["zero"]] == 1.0 and gains[by["8000/3199"]] == 1.0 and not limited[by["zero"]]                 # L = -inf
    assert not limited[by["25 LU apart"]] and gains[by["cropped"]] != 1.0
    crop = batch[by["cropped"]]
    assert crop["frames"] < crop["x"].shape[1]                                        # a tail past the frames exists and was compared


def test_gain_reaches_planes_that_lie_apart(batch):
    from sos_amd import audio_io
    some = [batch[4], batch[-4]]
    views = [torch.from_numpy(f["x"]).cuda() for f in some]
    stats = _measure(some, views)
    gains, _ = audio_io.loudness_gain_batch_device(views, stats["rows"], -24.0)
    for f, v, g in zip(some, views, gains.cpu().numpy()):
        assert np.array_equal(v.cpu().numpy().view(np.uint32), LR.apply_gain(f["x"], g).view(np.uint32)) and g != 1.0
        assert abs(float(g) / float(LR.gain(f["ref"]["lufs"], f["ref"]["peak"], -24.0)[0]) - 1.0) <= 2.0 ** -22


def test_a_device_row_outside_the_totals_is_skipped(batch):
    """The entry point itself with a device table that disagrees with the host's: the row gets no work and says so."""
    from sos_amd import _lib as L
    from sos_amd import metrics
    some = batch[:3]
    dev, views = _device_planes(some)
    tab = metrics.loudness_table([f["x"].shape[0] for f in some], [f["x"].shape[1] for f in some], [f["frames"] for f in some],
                                 [LR.hop(f["sr"]) for f in some])
    bad = tab.copy()
    bad[1, 1] = 1 << 40                                                               # a plane length no buffer holds
    h = L.lib()
    ws = torch.empty(h.sos_loudness_workspace_bytes(tab.ctypes.data_as(C.c_void_p), 3, 8), dtype=torch.uint8, device="cuda")
    coef = torch.from_numpy(np.stack([metrics.k_weighting(f["sr"]) for f in some])).cuda()
    w = torch.ones(sum(f["x"].shape[0] for f in some), dtype=torch.float64, device="cuda")
    rows = torch.full((3, 4), 5.0, dtype=torch.float64, device="cuda")
    rc = h.sos_loudness_batch_f64(L.ptr(dev), L.ptr(torch.from_numpy(bad).cuda()), tab.ctypes.data_as(C.c_void_p), 3, L.ptr(coef), L.ptr(w), 8,
                                  L.ptr(ws), ws.numel(), L.ptr(rows), L.stream_ptr())
    assert rc == 0, h.sos_last_error()
    rows = rows.cpu().numpy()
    assert np.isnan(rows[1, 0]) and rows[1, 2] == -1 and rows[1, 3] == -1
    assert _worst([some[0], some[2]], rows[[0, 2]]) <= BOUND_LU


# ------------------------------------------------------------------------------------------------ EBU Tech 3341 on the device
@pytest.mark.parametrize("case", [3, 5])
def test_tech_3341_on_the_device(case):
    """80 s and 60.1 s of stereo at 48 kHz: the carry runs across 6400 and 4808 chunks per plane."""
    segments, want = LR.TECH_3341[case]
    x = LR.sine(1000.0, 48000, segments, channels=2)
    ref = LR.measure(x, 48000)
    assert ref["margin"] > BOUND_LU
    from sos_amd import metrics
    got = metrics.loudness(torch.from_numpy(x).cuda(), 48000)
    print("Tech 3341 case %d: device %.9f LUFS, reference %.9f, difference %.3e LU" % (case, got["lufs"], ref["lufs"], abs(got["lufs"] - ref["lufs"])))
    assert (got["blocks"], got["blocks_abs"]) == (ref["blocks"], ref["blocks_abs"])
    assert abs(got["lufs"] - ref["lufs"]) <= BOUND_LU and abs(got["lufs"] - want) <= 0.1
