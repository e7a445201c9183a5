"""sos_true_peak_batch_f64 (csrc/loudness.hip) through metrics.true_peak_batch / true_peak / loudness_batch(true_peak=True) and
the true-peak ceiling of audio_io.loudness_gain_batch_device, against tests/r128_reference.py.
Bound.  The device and the reference multiply by the same float32 coefficients and read the same float32 samples; the reference
sums the 12 products in float64, the device with 12 fmaf in float32.  Every fmaf rounds once, by at most 2^-24 relative of a
partial sum that is itself at most sum_k |h_p[k]| |x[n + k]|, so one interpolated value differs by at most 12 * 2^-24 * sum_k
|h_p[k]| |x[n + k]| <= 12 * 2^-24 * S * max |x| with S = max_p sum_k |h_p[k]| (1.7251, taken from the coefficients below).  A
maximum moves by no more than its largest entry does, and widening the float32 maximum to float64 is exact; one more 2^-24 covers
the reference's own float64 roundings many times over: |peak - reference| <= 13 * 2^-24 * S * max |x| per file.
true peak >= sample peak holds exactly (phase 0 is the sample), and a maximum has no order: two calls give equal bits.
Shapes: one ragged group, planes back to back between sentinels so that most start off a 16-byte line: frames 0, 1, 5, 6, 11, 12,
13 (around the half length and the tap count), TILE - 1, TILE, TILE + 1, 2 TILE + 7; 1, 2, 3 and 64 channels; a peak in the last
sample of the last channel, one in the halo between two tiles; a spike just past `frames`; frames past the plane's end; silence;
the fs/4 sine sampled 45 degrees off its crests.  A second group of 300 short files walks the flat grid's file search."""
import ctypes as C

import numpy as np
import pytest
import torch

import loudness_reference as LR
import r128_reference as R

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
COEF = R.true_peak_filter_f32()
S = float(np.max(np.abs(COEF.astype(np.float64)).sum(axis=1)))


def _bound(x):
    return 13.0 * 2.0 ** -24 * S * (float(np.max(np.abs(x))) if x.size else 0.0)


def _add(files, name, x, frames=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    frames = x.shape[1] if frames is None else frames
    files.append(dict(name=name, x=x, frames=frames, ref=R.true_peak(x, frames), sample=float(np.max(np.abs(LR.extent(x, frames)), initial=0.0))))


@pytest.fixture(scope="module")
def group():
    from sos_amd import metrics
    tile = metrics.TRUE_PEAK_TILE
    rng = np.random.default_rng(20261021)
    files = []
    for j, n in enumerate((0, 1, 5, 6, 11, 12, 13, tile - 1, tile, tile + 1, 2 * tile + 7)):
        _add(files, "n=%d" % n, 0.3 * rng.standard_normal((1 + j % 3, n)), None)
    _add(files, "64 channels", 0.2 * rng.standard_normal((64, 37)))
    x = 0.01 * rng.standard_normal((3, tile + 1))
    x[2, -1] = 0.9
    _add(files, "last sample of the last channel", x)
    x = 0.01 * rng.standard_normal((1, 2 * tile + 7))
    x[0, tile - 3:tile + 1] = (0.8, -0.8, 0.8, -0.8)                                   # points n = tile - 1 on belong to the second tile
    _add(files, "between two tiles", x)
    x = 0.1 * rng.standard_normal((2, 501))
    x[:, 300] = 100.0
    _add(files, "spike past the frames", x, frames=300)
    x = 0.1 * rng.standard_normal((1, 301))
    x[0, -2:] = (0.7, -0.9)
    _add(files, "frames past the end", x, frames=341)
    _add(files, "zero", np.zeros((2, 101)))
    _add(files, "fs/4 at 45 degrees", R.faded_sine(4, 45.0))
    return files


def _device_planes(files, lead=3):
    flat = np.concatenate([np.full(lead, SENTINEL, np.float32)] + [f["x"].reshape(-1) for f in files] + [np.full(64, SENTINEL, np.float32)])
    dev = torch.from_numpy(flat).cuda()
    views, at = [], lead
    for f in files:
        views.append(dev[at:at + f["x"].size].view(f["x"].shape))
        at += f["x"].size
    return dev, views


def _check(files, got):
    worst = 0.0
    for f, v in zip(files, got):
        err, bound = abs(v - f["ref"]), _bound(LR.extent(f["x"], f["frames"]))
        print("%-34s device %.9g reference %.9g |difference| %.3e bound %.3e" % (f["name"], v, f["ref"], err, bound))
        assert err <= bound, f["name"]
        assert v >= f["sample"], (f["name"], v, f["sample"])                          # exactly: phase 0 is the sample
        worst = max(worst, err / bound if bound else 0.0)
    return worst


def test_one_ragged_group_is_the_reference(group):
    from sos_amd import metrics
    _, views = _device_planes(group)
    assert sum(v.storage_offset() % 4 != 0 for v in views) >= 8
    frames = [f["frames"] for f in group]
    got = metrics.true_peak_batch(views, frames)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (len(group),)
    host = got.cpu().numpy()
    print("largest |difference| / bound: %.3f" % _check(group, host))
    assert np.array_equal(host.astype(np.float32).astype(np.float64), host)           # a float32 maximum, widened
    by = {f["name"]: (f, v) for f, v in zip(group, host)}
    assert by["zero"][1] == 0.0 and by["n=0"][1] == 0.0
    assert by["spike past the frames"][1] < 1.0                                       # not even through the filter's reach
    sine, tp = by["fs/4 at 45 degrees"]
    assert abs(R.db(tp) + 6.02) <= 0.01 and abs(R.db(sine["sample"]) + 9.03) <= 0.01
    assert by["between two tiles"][1] > 0.8 and by["last sample of the last channel"][1] >= np.float32(0.9)
    again = metrics.true_peak_batch(views, frames)
    assert torch.equal(again.view(torch.int64), got.view(torch.int64))                # equal bits


def test_the_rows_of_loudness_batch_carry_it(group):
    from sos_amd import metrics
    some = [f for f in group if f["name"] in ("n=%d" % (metrics.TRUE_PEAK_TILE + 1), "fs/4 at 45 degrees", "zero")]
    _, views = _device_planes(some, lead=1)
    frames = [f["frames"] for f in some]
    plain = metrics.loudness_batch(views, 8000, frames=frames)
    got = metrics.loudness_batch(views, 8000, frames=frames, true_peak=True)
    assert set(plain) == {"lufs", "peak", "blocks", "blocks_abs", "rows"} and set(got) == set(plain) | {"true_peak", "rows_true"}
    assert torch.equal(got["rows"].view(torch.int64), plain["rows"].view(torch.int64))
    rows, rows_true, tp = got["rows"].cpu().numpy(), got["rows_true"].cpu().numpy(), got["true_peak"].cpu().numpy()
    assert np.array_equal(rows_true[:, [0, 2, 3]], rows[:, [0, 2, 3]], equal_nan=True) and np.array_equal(rows_true[:, 1], tp)
    assert np.array_equal(tp, metrics.true_peak_batch(views, frames).cpu().numpy())
    assert np.array_equal(rows[:, 1], [f["sample"] for f in some])
    _check(some, tp)


def test_three_hundred_short_files_on_the_flat_grid():
    from sos_amd import metrics
    rng = np.random.default_rng(7)
    files = []
    for i in range(300):
        n = int(rng.integers(0, 700))
        _add(files, "short %d" % i, 0.5 * rng.standard_normal((1 + i % 3, n)), None if i % 5 else max(n - 3, 0))
    _, views = _device_planes(files, lead=2)
    got = metrics.true_peak_batch(views, [f["frames"] for f in files]).cpu().numpy()
    for f, v in zip(files, got):
        assert abs(v - f["ref"]) <= _bound(LR.extent(f["x"], f["frames"])) and v >= f["sample"], f["name"]


def test_more_tiles_than_workgroups():
    """The grid stops at 2048 workgroups: with 2589 tiles a workgroup owns one or two consecutive tiles, and some of these pairs
    span two planes or two files (the walk from one file's last tile to the next file's first)."""
    from sos_amd import metrics
    tile = metrics.TRUE_PEAK_TILE
    rng = np.random.default_rng(11)
    files = []
    for name, ch, n in (("64 x 17 tiles", 64, 17 * tile - 6), ("one tile", 1, 99), ("50 x 30 tiles", 50, 29 * tile + 5)):
        x = (0.05 * rng.standard_normal((ch, n))).astype(np.float32)
        x[ch - 1, n - 2] = 0.6                                                       # the file's peak sits in its last tile
        _add(files, name, x)
    assert sum(f["x"].shape[0] * -(-(f["frames"] + 1) // tile) for f in files) == 64 * 17 + 1 + 50 * 30 > 2048
    _, views = _device_planes(files, lead=1)
    _check(files, metrics.true_peak_batch(views).cpu().numpy())


def test_one_clip_and_planes_apart(group):
    from sos_amd import metrics
    sine = next(f for f in group if f["name"] == "fs/4 at 45 degrees")
    assert abs(metrics.true_peak(sine["x"][0]) - sine["ref"]) <= _bound(sine["x"])
    assert abs(metrics.true_peak(torch.from_numpy(sine["x"]).cuda()) - sine["ref"]) <= _bound(sine["x"])
    one = metrics.loudness(sine["x"], 8000, true_peak=True)
    assert abs(one["true_peak"] - sine["ref"]) <= _bound(sine["x"]) and one["peak"] == sine["sample"]
    some = [group[9], group[12]]
    got = metrics.true_peak_batch([torch.from_numpy(f["x"]).cuda() for f in some]).cpu().numpy()
    _check(some, got)
    assert np.array_equal(metrics.true_peak_filter(), COEF) and metrics.true_peak_filter().dtype == np.float32


def test_empty_input_and_bad_arguments(group):
    from sos_amd import metrics
    empty = metrics.true_peak_batch([])
    assert empty.shape == (0,) and empty.dtype == torch.float64
    x = torch.zeros((2, 10), device="cuda")
    for bad in ([x.double()], [x[0]], [torch.zeros((65, 4), device="cuda")], [x.cpu().numpy()]):
        with pytest.raises(ValueError):
            metrics.true_peak_batch(bad)
    for frames in ([-1], [1, 2]):
        with pytest.raises(ValueError):
            metrics.true_peak_batch([x], frames)
    with pytest.raises(ValueError):
        metrics.true_peak(np.zeros((2, 2, 2), np.float32))
    with pytest.raises(RuntimeError):
        metrics.true_peak_batch([x.cpu()])


def test_a_device_row_outside_the_totals_reads_nan(group):
    from sos_amd import _lib as L
    from sos_amd import metrics
    some = group[3:6]
    dev, _ = _device_planes(some, lead=0)
    tab = metrics.loudness_table([f["x"].shape[0] for f in some], [f["x"].shape[1] for f in some], [f["frames"] for f in some], [1, 1, 1], 1)
    bad = tab.copy()
    bad[1, 1] = 1 << 40
    peaks = torch.full((3,), 5.0, dtype=torch.float64, device="cuda")
    h = L.lib()
    bad_dev, tab_dev, coef = torch.from_numpy(bad).cuda(), torch.from_numpy(tab).cuda(), torch.from_numpy(COEF).cuda()     # kept alive
    rc = h.sos_true_peak_batch_f64(L.ptr(dev), L.ptr(bad_dev), tab.ctypes.data_as(C.c_void_p), 3, L.ptr(coef), L.ptr(peaks), L.stream_ptr())
    assert rc == 0, h.sos_last_error()
    peaks_dev, peaks = peaks, peaks.cpu().numpy()
    assert np.isnan(peaks[1])
    _check([some[0], some[2]], peaks[[0, 2]])
    bad[1, 1] = -1                                                                    # the host refuses its own bad table
    assert h.sos_true_peak_batch_f64(L.ptr(dev), L.ptr(tab_dev), bad.ctypes.data_as(C.c_void_p), 3, L.ptr(coef), L.ptr(peaks_dev), L.stream_ptr()) == -22


def test_the_ceiling_bounds_the_true_peak_when_handed_rows_true():
    """g = min(10^((T - L) / 20), 10^(P / 20) / true peak): a loud target, so the ceiling binds.  g within 2^-22 relative of the
    reference's from the reference's own L and true peak (tests/test_gpu_loudness.py's bound; the device's true peak adds
    13 * 2^-24 * S relative of max |x| <= the peak).  The scaled file's true peak, by the reference on the planes read back: at most
    the ceiling times (1 + 2^-22 (g) + 2^-24 (x * g) + 13 * 2^-24 S (the measured peak)) -- the interpolation is linear."""
    from sos_amd import audio_io, metrics
    sr, ceiling, TARGET = 8000, -1.0, 6.0
    x = np.tile(R.faded_sine(4, 45.0, n=8192), (2, 1))
    y = (0.25 * np.random.default_rng(3).standard_normal((1, 8000))).astype(np.float32)
    refs = [LR.measure(v, sr) for v in (x, y)]
    tps = [R.true_peak(v) for v in (x, y)]
    planes = [torch.from_numpy(v).cuda() for v in (x, y)]
    got = metrics.loudness_batch(planes, sr, true_peak=True)
    by_sample = [LR.gain(r["lufs"], r["peak"], TARGET, ceiling)[0] for r in refs]
    gains, limited = audio_io.loudness_gain_batch_device(planes, got["rows_true"], TARGET, ceiling)
    slack = 2.0 ** -22 + 2.0 ** -24 + 13.0 * 2.0 ** -24 * S
    for v, r, tp, p, g, lim, gs in zip((x, y), refs, tps, planes, gains.cpu().numpy(), limited.cpu().numpy(), by_sample):
        g_ref, lim_ref = LR.gain(r["lufs"], tp, TARGET, ceiling)
        assert lim and lim_ref and abs(float(g) / float(g_ref) - 1.0) <= 2.0 ** -22 + 13.0 * 2.0 ** -24 * S
        after = R.true_peak(p.cpu().numpy())
        print("true peak %.4f dBTP after the gain (ceiling %.1f); a sample-peak ceiling would leave %.4f dBTP"
              % (R.db(after), ceiling, R.db(float(gs) * tp)))
        assert after <= 10.0 ** (ceiling / 20.0) * (1.0 + slack)
        assert np.array_equal(p.cpu().numpy(), LR.apply_gain(v, g))
    assert R.db(float(by_sample[0]) * tps[0]) > ceiling + 2.9                         # the sine: 3.01 dB over under the sample peak
