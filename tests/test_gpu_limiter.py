"""sos_limiter_batch_f32 (csrc/limiter.hip) through audio_io.limit_batch_device against tests/limiter_reference.py.
One ragged group, chosen for the kernel's edges: 1, 2, 3 and 64 channels; frames 0, 1, H, 2 H + 1, TILE - 1, TILE, TILE + 1 and
2 TILE + 4 H + 3; H = 1, 7, 240 and 1024 in ONE launch (5 ms at 200, 1400, 48000 and 204800 Hz); samples over the ceiling at t = 0,
at t = m - 1 and within H of either side of every tile edge; frames past the plane's end and short of it (with a spike past them,
which must pass untouched); odd plane lengths between sentinels, once from a buffer that starts three samples off a 16-byte line
(input and output lie differently: scalar loads) and once on a line (16-byte loads and stores).
What is observed.  The limiter returns y, not g.  s is made a power of two here (T - L = 20 log10 of 1, 2 or 4: float32 rounds the
power to it exactly, which the test asserts), and the last channel of every file with more than one channel is the constant 2^-20:
far below the other channels, so it never decides the envelope, and y = 2^-20 * (g * s) is exact -- that channel returns g bit for
bit.  The rows give the least g and the count of samples with g < 1 for every file.
Sample mode: y of every channel, g of every probe channel, the least g and the count EQUAL the reference.
True mode.  The device forms an interpolated point with 12 fmaf in float32, the reference sums in float64 and rounds the point
to float32 once.  Fmaf j rounds a partial sum of at most sum_{k <= j} |h[k]| max |x|, so the 12 of them move a point by at most
PARTIAL * 2^-24 * max |x| with PARTIAL = max_p sum_j sum_{k <= j} |h_p[k]| = 6.5 S (S = 1.7251, the absolute sum; both from the
coefficients below), the reference's rounding by at most S * 2^-24 * max |x|: the envelopes differ by at most 7.5 * 2^-24 * S * max |x|,
which leaves 5.5 of the 13 units of the existing true-peak test's bound d = 13 * 2^-24 * S * max |x| (the test asserts at least 2.5).
Both sides then apply the SAME float32 steps to their p: a = s p (2^-24 relative, which moves C / a < 1 by at most 2^-24), r rounded
(2^-25 below 1) and at the end g rounded (2^-25) -- 2^-23 + 2^-24 + 2^-24 = 2^-22 for the two sides together.  C / (s p) has slope at
most s / C where s p > C and meets 1 at s p = C, the floor only clips, and a minimum and a mean are 1-Lipschitz in their largest
entry (the float64 mean is exact): |g - g_ref| <= 7.5 * 2^-24 * S * max |x| * s / C + 2^-22.  A g below 1 on either side needs a > C
there, so s * S * max |x| / C >= 1 - 2^-20, and 2.5 of the spare units, 2.5 * 2^-24 * (s S max |x| / C), cover the 2^-23 by which
2^-22 exceeds the term asserted:
    |g - g_ref| <= s * 13 * 2^-24 * S * max |x| / C + 2^-23          (inputs keep s max |x| / C <= 8)
For a mono file (no probe) the same bound is carried to y: |y - y_ref| <= |x| s (bound + 2^-23).  The least g moves by the
bound too.  A file that is never over the ceiling equals loudness_gain_batch_device bit for bit, a file alone equals itself in the
batch, two calls give equal bits, and bad arguments are refused with SOS_EINVAL before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import limiter_reference as M
import r128_reference as R

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
CEILING = -1.0
MS = 5.0
RATE_OF = {1: 200, 7: 1400, 240: 48000, 1024: 204800}
PROBE = np.float32(2.0 ** -20)
COEF = R.true_peak_filter_f32().astype(np.float64)
S = float(np.max(np.abs(COEF).sum(axis=1)))
PARTIAL = float(np.max(np.cumsum(np.abs(COEF), axis=1).sum(axis=1)))
L0 = -20.0


def _file(name, x, H, s, frames=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.shape[0] > 1:
        x[-1, :] = PROBE
    return dict(name=name, x=x, H=H, rate=RATE_OF[H], s=float(s), target=L0 + 20.0 * np.log10(float(s)),
                frames=x.shape[1] if frames is None else frames)


def _spiky(rng, ch, n, H, s, tile, level=0.02):
    """Noise far under the ceiling with single samples over it at the places the kernel can get wrong."""
    c = float(M.ceiling(CEILING))
    x = level * rng.standard_normal((ch, n))
    for k in range(1, 4):
        edge = k * tile
        for t in (edge - H, edge - 1 - H // 2, edge - 1, edge, edge + H // 2, edge + H - 1):
            if 0 <= t < n:
                x[rng.integers(0, max(ch - 1, 1)), t] = rng.choice((-1.0, 1.0)) * rng.uniform(1.1, 7.0) * c / s
    for t in (0, n - 1):
        if n:
            x[0, t] = rng.uniform(1.5, 6.0) * c / s
    return x


@pytest.fixture(scope="module")
def group():
    from sos_amd import audio_io
    tile = audio_io.LIMITER_TILE
    rng = np.random.default_rng(20261021)
    files, hs = [], (1, 7, 240, 1024)
    sizes = (("0", lambda H: 0, (1,)), ("1", lambda H: 1, (7,)), ("H", lambda H: H, (240,)), ("2H+1", lambda H: 2 * H + 1, (1024,)),
             ("tile-1", lambda H: tile - 1, (1,)), ("tile", lambda H: tile, (7, 240)), ("tile+1", lambda H: tile + 1, (1024,)),
             ("2tile+4H+3", lambda H: 2 * tile + 4 * H + 3, (240, 1024)))
    for j, (kind, n_of, its) in enumerate(sizes):
        for H in its:
            s = (1.0, 2.0, 4.0)[(j + H) % 3]
            files.append(_file("n=%s H=%d" % (kind, H), _spiky(rng, 1 + (j + H) % 3, n_of(H), H, s, tile), H, s))
    files.append(_file("64 channels", _spiky(rng, 64, tile + 37, 7, 2.0, tile), 7, 2.0))
    x = _spiky(rng, 2, tile + 1, 240, 2.0, tile)
    files.append(_file("frames past the end", x, 240, 2.0, frames=tile + 51))
    x = _spiky(rng, 3, 2 * 240 + 101, 240, 1.0, tile)
    x[0, 2 * 240 + 4] = 5.0                                                            # past the frames: read as 0, copied as it is
    files.append(_file("frames short of the end", x, 240, 1.0, frames=2 * 240 + 1))
    files.append(_file("never over", 0.02 * rng.standard_normal((3, tile + 77)), 240, 2.0))
    files.append(_file("fs/4 at 45 degrees", R.faded_sine(4, 45.0, amp=0.5), 7, 4.0))
    files.append(_file("fs/4 stereo, long look-ahead", np.tile(R.faded_sine(4, 45.0, amp=0.6, n=tile + 600), (3, 1)), 1024, 2.0))
    for f in files:
        assert M.lookahead(MS, f["rate"]) == f["H"] and M.to_target(L0, f["target"]) == np.float32(f["s"]), f["name"]
        ext = f["x"][:, :min(f["frames"], f["x"].shape[1])]
        f["max"] = float(np.max(np.abs(ext), initial=0.0))
        assert f["s"] * f["max"] / float(M.ceiling(CEILING)) <= 8.0, f["name"]
        f["ref"] = {tp: M.limit(f["x"], f["s"], CEILING, f["H"], f["frames"], tp) for tp in (False, True)}
    assert {f["x"].shape[0] for f in files} == {1, 2, 3, 64} and {f["H"] for f in files} == set(hs)
    assert sum(f["ref"][False]["samples"] > 0 for f in files) >= len(files) - 4
    return files


def _device_planes(files, lead):
    flat = np.concatenate([np.full(lead, SENTINEL, np.float32)] + [f["x"].reshape(-1) for f in files] + [np.full(64, SENTINEL, np.float32)])
    dev = torch.from_numpy(flat).cuda()
    views, at = [], lead
    for f in files:
        views.append(dev[at:at + f["x"].size].view(f["x"].shape))
        at += f["x"].size
    return dev, views


def _rows(files):
    """The stats rows {L, sample peak, -, -} the limiter and the gain read."""
    return torch.from_numpy(np.asarray([[L0, f["max"], 1.0, 1.0] for f in files], dtype=np.float64)).cuda()


def _run(files, lead, true_peak):
    from sos_amd import audio_io
    _, views = _device_planes(files, lead)
    targets = torch.from_numpy(np.asarray([f["target"] for f in files], dtype=np.float64)).cuda()
    out, rows = audio_io.limit_batch_device(views, _rows(files), targets, CEILING, rates=[f["rate"] for f in files], lookahead_ms=MS,
                                            frames=[f["frames"] for f in files], true_peak=true_peak)
    assert rows.is_cuda and rows.dtype == torch.float64 and rows.shape == (len(files), 4)
    assert all(o.shape == v.shape and o.dtype == torch.float32 for v, o in zip(views, out))
    return [o.cpu().numpy() for o in out], rows.cpu().numpy(), out, rows


@pytest.fixture(scope="module")
def runs(group):
    return {(lead, tp): _run(group, lead, tp) for lead in (3, 0) for tp in (False, True)}


def test_the_target_gain_is_the_reference_within_an_ulp(group, runs):
    rows = runs[(3, False)][1]
    for f, row in zip(group, rows):
        assert abs(row[0] - f["s"]) <= np.spacing(np.float32(f["s"])) and row[3] == 0.0, f["name"]
        assert row[0] == f["s"], f["name"]                                            # a power of two: the probe returns g itself


@pytest.mark.parametrize("lead", (3, 0))
def test_sample_mode_equals_the_reference(group, runs, lead):
    ys, rows, _, _ = runs[(lead, False)]
    c = float(M.ceiling(CEILING))
    for f, y, row in zip(group, ys, rows):
        ref = f["ref"][False]
        assert np.array_equal(y, ref["y"]), f["name"]
        m = min(f["frames"], f["x"].shape[1])
        if f["x"].shape[0] > 1:
            assert np.array_equal(y[-1, :m] / (PROBE * np.float32(f["s"])), ref["g"]), f["name"]
        assert row[1] == ref["min_g"] and row[2] == ref["samples"], (f["name"], row, ref["min_g"], ref["samples"])
        assert np.max(np.abs(y[:, :m]), initial=0.0) <= c * (1.0 + 3.0 * 2.0 ** -24), f["name"]
        assert np.array_equal(y[:, m:], f["x"][:, m:]), f["name"]
    print("files with a limited sample: %d of %d; least g %.4f" % (sum(r[2] > 0 for r in rows), len(group), rows[:, 1].min()))


@pytest.mark.parametrize("lead", (3, 0))
def test_true_mode_is_within_the_derived_bound(group, runs, lead):
    assert 13.0 * S - (PARTIAL + S) >= 2.5 * S                                        # the docstring's margin for the float32 steps
    ys, rows, _, _ = runs[(lead, True)]
    c = float(M.ceiling(CEILING))
    worst = 0.0
    for f, y, row in zip(group, ys, rows):
        ref = f["ref"][True]
        bound = f["s"] * 13.0 * 2.0 ** -24 * S * f["max"] / c + 2.0 ** -23
        m = min(f["frames"], f["x"].shape[1])
        if f["x"].shape[0] > 1:
            g = y[-1, :m].astype(np.float64) / (float(PROBE) * f["s"])
            err = float(np.max(np.abs(g - ref["g"]), initial=0.0))
            assert err <= bound, (f["name"], err, bound)
            worst = max(worst, err / bound)
        err = np.abs(y.astype(np.float64) - ref["y"])
        assert np.all(err <= np.abs(f["x"]) * f["s"] * (bound + 2.0 ** -23)), f["name"]
        assert abs(row[1] - ref["min_g"]) <= bound, f["name"]
        assert np.array_equal(y[:, m:], f["x"][:, m:]), f["name"]
    print("largest |g - reference| / bound: %.4f" % worst)
    by = {f["name"]: (f, y) for f, y in zip(group, ys)}
    f, y = by["fs/4 at 45 degrees"]
    sample = runs[(lead, False)][0][[g["name"] for g in group].index(f["name"])]
    print("fs/4 burst: true peak %.5f after the true form, %.5f after the sample form, ceiling %.5f" % (R.true_peak(y), R.true_peak(sample), c))
    assert R.true_peak(y) <= c + 6.0 / (2 * f["H"] + 1) * S * f["s"] * f["max"]


def test_a_file_never_over_the_ceiling_is_the_plain_gain(group, runs):
    from sos_amd import audio_io
    i = [f["name"] for f in group].index("never over")
    f = group[i]
    x = torch.from_numpy(f["x"]).cuda()
    gains, limited = audio_io.loudness_gain_batch_device([x], _rows([f]), f["target"], CEILING)
    assert not bool(limited[0]) and float(gains[0]) == f["s"]
    for lead in (3, 0):
        for tp in (False, True):
            assert np.array_equal(runs[(lead, tp)][0][i], x.cpu().numpy()) and runs[(lead, tp)][1][i, 2] == 0.0


def test_a_file_alone_and_a_second_call_give_equal_bits(group, runs):
    i = [f["name"] for f in group].index("n=2tile+4H+3 H=240")
    for tp in (False, True):
        ys, rows, out, rows_dev = runs[(3, tp)]
        alone = _run([group[i]], 1, tp)
        assert np.array_equal(alone[0][0].view(np.int32), ys[i].view(np.int32)) and np.array_equal(alone[1][0], rows[i])
        again = _run(group, 3, tp)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again[2], out))
        assert torch.equal(again[3].view(torch.int64), rows_dev.view(torch.int64))


def test_bad_arguments_launch_nothing(group):
    from sos_amd import _lib as L
    from sos_amd import audio_io
    some = group[3:6]
    dev, views = _device_planes(some, 0)
    n = sum(f["x"].size for f in some)
    tab = np.zeros((3, 8), dtype=np.int64)
    tab[:, 0] = np.cumsum([0] + [f["x"].size for f in some[:-1]])
    tab[:, 1], tab[:, 2], tab[:, 3], tab[:, 4] = [f["x"].shape[1] for f in some], [f["x"].shape[0] for f in some], [f["frames"] for f in some], 7
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    rows = torch.full((3, 4), 5.0, dtype=torch.float64, device="cuda")
    stats, targets = _rows(some), torch.full((3,), L0, dtype=torch.float64, device="cuda")
    tab_dev = torch.from_numpy(tab).cuda()
    h = L.lib()

    def call(host, device=tab_dev, planes=dev, ceiling=CEILING, to=out):
        return h.sos_limiter_batch_f32(L.ptr(planes) if planes is not None else None, L.ptr(to), L.ptr(device), host.ctypes.data_as(C.c_void_p), 3,
                                       L.ptr(stats), L.ptr(targets), ceiling, 0, None, L.ptr(rows), L.stream_ptr())
    for col, value in ((4, 0), (4, 1025), (1, -1), (0, n), (2, 65), (3, -1)):
        bad = tab.copy()
        bad[1, col] = value
        assert call(bad) == -22 and b"file 1" in h.sos_last_error(), (col, value)
    assert call(tab, planes=None) == -22 and call(tab, ceiling=0.5) == -22 and call(tab, to=dev) == -22
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((rows == 5.0).all())                # nothing ran
    bad = tab.copy()
    bad[1, 1] = 1 << 40                                                               # the DEVICE table alone is wrong: that row is skipped
    bad_dev = torch.from_numpy(bad).cuda()
    assert call(tab, device=bad_dev) == 0, h.sos_last_error()
    got = rows.cpu().numpy()
    assert np.isnan(got[1, 0]) and got[1, 2] == -1.0 and got[0, 0] == 1.0 and got[2, 0] == 1.0
    x = views[0]
    for kw in (dict(rates=[8000], lookahead_ms=0.0), dict(rates=[8000], lookahead_ms=float("nan")), dict(rates=[100]), dict(rates=[300000]),
               dict(rates=[8000, 8000]), dict()):
        with pytest.raises(ValueError):
            audio_io.limit_batch_device([x], stats[:1], L0, CEILING, **kw)
    with pytest.raises(ValueError):
        audio_io.limit_batch_device([x], stats[:1], L0, 1.0, rates=[8000])
    empty = audio_io.limit_batch_device([], torch.zeros((0, 4), dtype=torch.float64, device="cuda"), L0, CEILING, rates=[])
    assert empty[0] == [] and empty[1].shape == (0, 4)
