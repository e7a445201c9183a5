"""sos_loudness_range_batch_f64 (csrc/loudness.hip) through metrics.loudness_batch / loudness(loudness_range=True), against
tests/r128_reference.py (itself held against stepped sines in tests/test_r128_reference.py).
Bounds.  `windows`: equality.  LRA, max_momentary, max_short_term: 1e-6 LU, the bound tests/test_gpu_loudness.py holds `lufs` to --
both sides are float64 on the same float32 samples and differ in the order of their sums only (the chunked scan of the filter, hop
sums added per chunk and then per window), about 1e-14 relative, where 1e-6 LU is 2.3e-7 relative in energy.  A difference of that
size could still move a window across a gate and with it a rank, so the test asserts first, ON THE REFERENCE alone, that no window
of any input lies within 1e-3 LU of either of its gates (range_margin).
Inputs: 1 kHz sines whose level steps between segments plus seeded noise bursts, at 8000, 11025 (hop 1103: no whole number of
hops in a second) and 44100 Hz; 2.5 s (no window), exactly 30 hops (one window), 30 hops + 1 sample, 10 s and 45 s; mono, stereo and
three channels weighted [1, 1.41, 0]; one file with a segment below the relative gate and one below the absolute gate; split 1 and 8."""
import ctypes as C

import numpy as np
import pytest
import torch

import loudness_reference as LR
import r128_reference as R

pytestmark = pytest.mark.gpu
BOUND_LU, MARGIN_LU = 1e-6, 1e-3
LAYOUTS = ((1, None), (2, None), (3, [1.0, 1.41, 0.0]))
KEYS = ("lra", "max_momentary", "max_short_term")


def _signal(rng, sr, n, ch, levels):
    """A 1 kHz sine stepping through `levels` (dBFS) in equal segments, a burst of noise 12 dB below it in every second one."""
    edges = np.linspace(0, n, len(levels) + 1).astype(np.int64)
    amp = np.zeros(n)
    for k, db in enumerate(levels):
        amp[edges[k]:edges[k + 1]] = 10.0 ** (db / 20.0)
    t = np.arange(n) / sr
    x = np.stack([amp * np.sin(2.0 * np.pi * 1000.0 * t + 0.7 * c) for c in range(ch)])
    for k in range(1, len(levels), 2):
        a, b = edges[k], edges[k + 1]
        x[:, a:b] += 0.25 * amp[a:b] * rng.standard_normal((ch, b - a))
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(20261022)
    files = []

    def add(name, x, sr, weights=None, frames=None):
        f = dict(name=name, x=np.ascontiguousarray(x), sr=sr, weights=weights, frames=x.shape[1] if frames is None else frames)
        f["ref"] = R.measure(f["x"], sr, weights, f["frames"])
        files.append(f)

    k = 0
    for sr in (8000, 11025, 44100):
        h = LR.hop(sr)
        for n, levels in ((int(2.5 * sr), (-20.0, -26.0)), (30 * h, (-18.0, -23.0, -29.0)), (30 * h + 1, (-31.0, -20.0)),
                          (10 * sr, (-20.0, -33.0, -24.0, -17.0, -28.0)), (45 * sr, (-23.0, -35.0, -19.0, -41.0, -27.0, -15.0, -30.0))):
            ch, w = LAYOUTS[k % 3]
            add("%d Hz, %d samples, %d ch" % (sr, n, ch), _signal(rng, sr, n, ch, levels), sr, w)
            k += 1
    add("below the relative gate", _signal(rng, 8000, 40 * 8000, 2, (-20.0, -52.0, -22.0, -49.0)), 8000)
    add("below the absolute gate", _signal(rng, 11025, 30 * 11025, 1, (-84.0, -21.0, -30.0)), 11025)
    add("cropped", _signal(rng, 8000, 12 * 8000, 1, (-20.0, -30.0, -25.0)), 8000, frames=12 * 8000 - 4321)
    return files


def _measure(files, **kw):
    from sos_amd import metrics
    planes = [torch.from_numpy(f["x"]).cuda() for f in files]
    return metrics.loudness_batch(planes, [f["sr"] for f in files], [f["weights"] for f in files], [f["frames"] for f in files], **kw)


def _worst(files, got):
    host = {k: got[k].cpu().numpy() for k in KEYS + ("windows",)}
    worst = 0.0
    for i, f in enumerate(files):
        ref = f["ref"]
        assert int(host["windows"][i]) == ref["windows"], (f["name"], host["windows"][i], ref["windows"])
        for k in KEYS:
            if np.isfinite(ref[k]):
                worst = max(worst, abs(host[k][i] - ref[k]))
                assert abs(host[k][i] - ref[k]) <= BOUND_LU, (f["name"], k, host[k][i], ref[k])
            else:
                assert host[k][i] == ref[k], (f["name"], k, host[k][i])
    return worst


def test_the_reference_of_the_batch_is_clear_of_its_gates(batch):
    """Before the device is looked at: every window is at least 1e-3 LU from both gates; both gates drop windows somewhere."""
    for f in batch:
        assert f["ref"]["range_margin"] >= MARGIN_LU, (f["name"], f["ref"]["range_margin"])
    by = {f["name"]: f for f in batch}
    for name in ("below the relative gate", "below the absolute gate"):
        f = by[name]
        assert 0 < f["ref"]["windows"] < f["frames"] // LR.hop(f["sr"]) - 29, name
    _, l = R.short_term(by["below the absolute gate"]["x"], 11025)
    assert np.any(l <= -70.0)
    assert [f["ref"]["windows"] for f in batch[:3]] == [0, 1, 1] and batch[0]["ref"]["max_short_term"] == -np.inf
    assert batch[0]["ref"]["lra"] == 0.0 and batch[1]["ref"]["lra"] == 0.0 and batch[4]["ref"]["lra"] > 3.0


@pytest.mark.parametrize("split", [1, 8])
def test_one_ragged_call_is_the_reference(batch, split):
    got = _measure(batch, split=split, loudness_range=True)
    for k in KEYS:
        assert got[k].is_cuda and got[k].dtype == torch.float64 and got[k].shape == (len(batch),)
    assert got["windows"].dtype == torch.int64
    worst = _worst(batch, got)
    print("split %d: largest difference of LRA / the maxima over %d files: %.3e LU (bound %.0e)" % (split, len(batch), worst, BOUND_LU))
    again = _measure(batch, split=split, loudness_range=True)
    for k in KEYS:
        assert torch.equal(again[k].view(torch.int64), got[k].view(torch.int64))      # fixed order of every sum: equal bits


def test_without_the_flags_the_call_is_what_it_was(batch):
    some = batch[:5]
    plain, both = _measure(some), _measure(some, true_peak=True, loudness_range=True)
    assert set(plain) == {"lufs", "peak", "blocks", "blocks_abs", "rows"}
    assert set(both) == set(plain) | {"true_peak", "rows_true", "lra", "max_momentary", "max_short_term", "windows"}
    assert torch.equal(plain["rows"].view(torch.int64), both["rows"].view(torch.int64))
    for k in plain:
        assert torch.equal(plain[k], both[k])


@pytest.mark.parametrize("levels,want", [((-20.0, -30.0), 10.0), ((-20.0, -15.0), 5.0), ((-40.0, -20.0), 20.0),
                                         ((-50.0, -35.0, -20.0, -35.0, -50.0), 15.0)])
def test_stepped_sines_read_their_level_difference(levels, want):
    from sos_amd import metrics
    x = LR.sine(1000.0, 8000, [(db, 20.0) for db in levels], channels=2)
    ref = R.measure(x, 8000)
    assert ref["range_margin"] >= MARGIN_LU
    got = metrics.loudness(x, 8000, loudness_range=True)
    print("%s: LRA %.9f LU (reference %.9f), %d windows" % (levels, got["lra"], ref["lra"], got["windows"]))
    assert got["windows"] == ref["windows"] and abs(got["lra"] - ref["lra"]) <= BOUND_LU and abs(got["lra"] - want) <= 0.01
    assert abs(got["max_momentary"] - ref["max_momentary"]) <= BOUND_LU and abs(got["max_short_term"] - ref["max_short_term"]) <= BOUND_LU
    assert set(got) == {"lufs", "peak", "blocks", "blocks_abs", "lra", "max_momentary", "max_short_term", "windows"}


def test_a_device_row_outside_the_totals_is_skipped(batch):
    from sos_amd import _lib as L
    from sos_amd import metrics
    some = batch[:3]
    dev = torch.from_numpy(np.concatenate([f["x"].reshape(-1) for f in some])).cuda()
    tab = metrics.loudness_table([f["x"].shape[0] for f in some], [f["x"].shape[1] for f in some], [f["frames"] for f in some],
                                 [LR.hop(f["sr"]) for f in some])
    bad = tab.copy()
    bad[1, 1] = 1 << 40
    h = L.lib()
    ws = torch.empty(h.sos_loudness_workspace_bytes(tab.ctypes.data_as(C.c_void_p), 3, 8), dtype=torch.uint8, device="cuda")
    need = h.sos_loudness_range_workspace_bytes(tab.ctypes.data_as(C.c_void_p), 3)
    assert need >= 16 * sum(f["x"].shape[0] * -(-f["frames"] // LR.hop(f["sr"])) for f in some)
    rw = torch.empty(need, dtype=torch.uint8, device="cuda")
    coef = torch.from_numpy(np.stack([metrics.k_weighting(f["sr"]) for f in some])).cuda()
    w = torch.from_numpy(np.concatenate([np.ones(f["x"].shape[0]) if f["weights"] is None else np.asarray(f["weights"]) for f in some])).cuda()
    rows = torch.empty((3, 4), dtype=torch.float64, device="cuda")
    out = torch.full((3, 4), 5.0, dtype=torch.float64, device="cuda")
    bad_dev = torch.from_numpy(bad).cuda()
    host = tab.ctypes.data_as(C.c_void_p)
    assert h.sos_loudness_batch_f64(L.ptr(dev), L.ptr(bad_dev), host, 3, L.ptr(coef), L.ptr(w), 8, L.ptr(ws), ws.numel(), L.ptr(rows),
                                    L.stream_ptr()) == 0, h.sos_last_error()
    assert h.sos_loudness_range_batch_f64(L.ptr(bad_dev), host, 3, L.ptr(w), 8, L.ptr(ws), ws.numel(), L.ptr(rw), rw.numel(), L.ptr(out),
                                          L.stream_ptr()) == 0, h.sos_last_error()
    out = out.cpu().numpy()
    assert np.all(np.isnan(out[1, :3])) and out[1, 3] == -1
    for i in (0, 2):
        ref = some[i]["ref"]
        assert out[i, 3] == ref["windows"] and abs(out[i, 1] - ref["max_momentary"]) <= BOUND_LU
    spare = torch.empty((3, 4), dtype=torch.float64, device="cuda")                   # a range buffer one line too small: SOS_ENOSPC
    assert h.sos_loudness_range_batch_f64(L.ptr(bad_dev), host, 3, L.ptr(w), 8, L.ptr(ws), ws.numel(), L.ptr(rw), rw.numel() - 256,
                                          L.ptr(spare), L.stream_ptr()) == -28
