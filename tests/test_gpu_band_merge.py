"""csrc/band_merge.hip on the device: sos_resample_merge_batch_f32 and sos_band_gain_batch_f32 through
audio_io.resample_merge_batch_device / band_gains_batch_device, and recordings.denoise_recordings(high_band=) end to end.
The merge's two resamplings are asked for the BITS of resample_batch_device, so with g = 1 the bound is equality with the f32
numpy expression (x - ra) + rb; with gains it is 2^-22 (|x - ra| + |rb|) against tests/band_reference.py fed the device's ra, rb
and s (g <= 1 is off by at most one f32 ulp, x - ra is rounded once, and there is one final rounding: (2^-23 + 2 * 2^-24) |x - ra|
+ 2^-24 |rb| at most).  The gains are float64 sums in no fixed order, rounded once to f32: 4 * 2^-24 on values within 0 .. 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_reference as B
import pcm_reference as R
from oracle import nets as onet

pytestmark = pytest.mark.gpu
SR, HOP = 14000, 158
SECONDS = dict(window_seconds=2.0, context_seconds=0.5)
# native lengths: under one tile of 4096 outputs, one sample over a tile, several tiles, an m that is no hop multiple
LENGTHS = (513, 4097, 9001, 30000)
CANARY = 64


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.int32)


def _fit(v, n):
    """A downloaded resampling cut or zero-filled to n frames, as the encode does."""
    out = np.zeros(n, dtype=np.float32)
    out[:min(n, len(v))] = v[:n]
    return out


def _cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()


@pytest.fixture(scope="module", params=[48000, 44100])
def batch(request):
    """A ragged batch at one rate: x random, a = x at 14 kHz (the device's), b random and unrelated to a, m' the hop multiple the
    networks would return (at 48 kHz the shortest clip has 150 samples, less than a hop: 143 there); ra, rb = resample_batch_device's
    outputs on the host, fitted to n; s = random gains with runs of exact 0 and 1.  Computed once and left unchanged."""
    from sos_amd import audio_io
    rate = request.param
    rng = np.random.default_rng(rate)
    xs = [_cuda(rng.uniform(-1, 1, n)) for n in LENGTHS]
    As = [t.clone() for t in audio_io.resample_batch_device(xs, rate, SR)]
    ms = [t.numel() for t in As]
    mps = [HOP * (m // HOP) if m >= HOP else m - 7 for m in ms]
    assert [m for m in ms if m % HOP] and all(1 <= p <= m for p, m in zip(mps, ms))
    bs = [_cuda(rng.uniform(-1, 1, p)) for p in mps]
    ra = [_fit(t.cpu().numpy(), n) for t, n in zip(audio_io.resample_batch_device(As, SR, rate), LENGTHS)]
    rb = [_fit(t.cpu().numpy(), n) for t, n in zip(audio_io.resample_batch_device(bs, SR, rate), LENGTHS)]
    ss = []
    for m in ms:
        s = rng.uniform(0, 1, -(-m // HOP)).astype(np.float32)
        if len(s) > 8:
            s[1:4], s[5:8] = 0.0, 1.0
        ss.append(s)
    return dict(rate=rate, xs=xs, As=As, bs=bs, ms=ms, mps=mps, ra=ra, rb=rb, ss=ss, x=[t.cpu().numpy() for t in xs])


def _raw_merge(batch, gains=None):
    """The entry point itself on buffers of the test's own: out pre-filled with NaN between two canaries.  -> the whole buffer."""
    from sos_amd import _lib as L
    from sos_amd import audio_io
    n, m, mp = (np.asarray(v, dtype=np.int64) for v in (LENGTHS, batch["ms"], batch["mps"]))
    J = -(-m // HOP)
    off = lambda v: np.cumsum(v) - v                             # noqa: E731
    tab = np.ascontiguousarray(np.stack([off(n), n, off(m), m, off(mp), mp, off(J), J, off(-(-n // L.RESAMPLE_CHUNK))]), dtype=np.int64)
    tab_dev = torch.from_numpy(tab).cuda()
    x, a, b = torch.cat(batch["xs"]), torch.cat(batch["As"]), torch.cat(batch["bs"])
    s = torch.cat([_cuda(g) for g in gains]) if gains is not None else None
    ratio = float(batch["rate"]) / SR
    win, num_table = audio_io._filter_on(x.device, ratio, "kaiser_best")
    buf = torch.full((CANARY + int(n.sum()) + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:CANARY] = 12345.0
    buf[-CANARY:] = -54321.0
    L.check(L.lib().sos_resample_merge_batch_f32(L.ptr(x), L.ptr(a), L.ptr(b), L.ptr(s), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p),
                                                 len(n), ratio, L.ptr(win), win.numel(), num_table, HOP, L.ptr(buf[CANARY:]),
                                                 L.stream_ptr()), "sos_resample_merge_batch_f32")
    return buf.cpu().numpy()


def test_merge_without_gains_is_the_f32_expression_bit_for_bit_and_stays_inside_out(batch):
    from sos_amd import audio_io
    buf = _raw_merge(batch)
    assert np.all(buf[:CANARY] == 12345.0) and np.all(buf[-CANARY:] == -54321.0), "a canary around out was overwritten"
    body = buf[CANARY:-CANARY]
    assert not np.isnan(body).any(), "an output frame was not written"
    want = [(x - ra) + rb for x, ra, rb in zip(batch["x"], batch["ra"], batch["rb"])]         # f32 numpy: each step rounded once
    assert want[0].dtype == np.float32
    assert np.array_equal(_bits(body), _bits(np.concatenate(want)))
    outs = audio_io.resample_merge_batch_device(batch["xs"], batch["As"], batch["bs"], SR, batch["rate"])
    assert [tuple(o.shape) for o in outs] == [(n,) for n in LENGTHS]
    assert np.array_equal(_bits(torch.cat(outs).cpu().numpy()), _bits(body))
    assert outs[1].data_ptr() == outs[0].data_ptr() + 4 * LENGTHS[0]                          # back to back in one buffer


def test_a_clip_gets_the_same_bits_alone_and_in_any_batch_position(batch):
    from sos_amd import audio_io
    go = lambda idx: [o.cpu().numpy() for o in audio_io.resample_merge_batch_device(                              # noqa: E731
        [batch["xs"][i] for i in idx], [batch["As"][i] for i in idx], [batch["bs"][i] for i in idx], SR, batch["rate"],
        gains=[_cuda(batch["ss"][i]) for i in idx])]
    whole = go([0, 1, 2, 3])
    for order in ([3, 2, 1, 0], [2, 0, 3, 1]):
        for i, o in zip(order, go(order)):
            assert np.array_equal(_bits(o), _bits(whole[i])), (order, i)
    for i in range(len(LENGTHS)):
        assert np.array_equal(_bits(go([i])[0]), _bits(whole[i])), i


def test_merge_with_gains_is_within_the_rounding_bound_of_the_reference(batch):
    body = _raw_merge(batch, batch["ss"])[CANARY:-CANARY]
    at = 0
    for x, ra, rb, s, n in zip(batch["x"], batch["ra"], batch["rb"], batch["ss"], LENGTHS):
        g = B.interp(s, n, SR, batch["rate"], HOP)
        ref = B.merge(x, ra, rb, g)
        bound = 2.0 ** -22 * (np.abs(x.astype(np.float64) - ra) + np.abs(rb.astype(np.float64)))
        err = np.abs(body[at:at + n].astype(np.float64) - ref)
        print(batch["rate"], n, "max error / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound)
        at += n


def test_unit_gains_are_the_merge_without_gains_and_zero_gains_the_plain_resampling(batch):
    none = _raw_merge(batch)
    ones = _raw_merge(batch, [np.ones_like(s) for s in batch["ss"]])
    zeros = _raw_merge(batch, [np.zeros_like(s) for s in batch["ss"]])
    assert np.array_equal(_bits(ones), _bits(none))
    assert np.array_equal(_bits(zeros[CANARY:-CANARY]), _bits(np.concatenate(batch["rb"])))


def _altered_device_rows(with_gains, n, mp, cases_of):
    """One good call of sos_resample_merge_batch_f32 over clips of n native frames (m = ceil(n / ratio), m' = mp) at 14 -> 48 kHz,
    then one call per case of cases_of(tab, n, m, mp, J, totals) = (what, row of the table, clip, value, the first output of the
    clip that must keep the canary; None: the field is not read) with that one entry of the DEVICE table altered."""
    from sos_amd import _lib as L
    from sos_amd import audio_io
    SPARE, canary, ratio = 16, -77.0, 48000.0 / SR
    n, mp = np.asarray(n, dtype=np.int64), np.asarray(mp, dtype=np.int64)
    m = np.asarray([int(np.ceil(v / ratio)) for v in n], dtype=np.int64)
    J = -(-m // HOP)
    off = lambda v: np.cumsum(v) - v                                                 # noqa: E731
    tab = np.ascontiguousarray(np.stack([off(n), n, off(m), m, off(mp), mp, off(J), J, off(-(-n // L.RESAMPLE_CHUNK))]), dtype=np.int64)
    tx, ta, tb, tg = (int(v.sum()) for v in (n, m, mp, J))
    tiles = int((-(-n // L.RESAMPLE_CHUNK)).sum())
    rng = np.random.default_rng(9)
    x, a, b = (_cuda(rng.uniform(-1, 1, t + SPARE)) for t in (tx, ta, tb))
    s = _cuda(rng.uniform(0, 1, tg + SPARE)) if with_gains else None
    win, num_table = audio_io._filter_on(x.device, ratio, "kaiser_best")

    def run(d_tab):
        out = torch.full((tx + SPARE,), canary, dtype=torch.float32, device="cuda")
        rc = L.lib().sos_resample_merge_batch_f32(L.ptr(x), L.ptr(a), L.ptr(b), L.ptr(s), L.ptr(torch.from_numpy(d_tab).cuda()),
                                                  tab.ctypes.data_as(C.c_void_p), len(n), ratio, L.ptr(win), win.numel(), num_table,
                                                  HOP, L.ptr(out), L.stream_ptr())
        return rc, out.cpu().numpy()

    rc, base = run(tab)
    assert rc == 0 and not (base[:tx] == canary).any() and (base[tx:] == canary).all()
    for what, row, clip, value, kept_from in cases_of(tab, n, m, mp, J, (tx, ta, tb, tg)):
        d_tab = tab.copy()
        d_tab[row, clip] = value
        xo, nn, ao, mm, bo, pp, go, jj, t0 = (int(v) for v in d_tab[:, clip])
        # what a kernel that followed the row would touch lies inside the allocations
        assert 0 <= xo and xo + max(nn, 0) <= tx + SPARE and 0 <= ao and ao + max(mm, 0) <= ta + SPARE, what
        assert 0 <= bo and bo + max(pp, 0) <= tb + SPARE and 0 <= go and go + max(jj, 0) <= tg + SPARE and 0 <= t0 < tiles, what
        rc, got = run(d_tab)
        assert rc == 0, what
        lo, hi = int(tab[0, clip]), int(tab[0, clip] + n[clip])
        assert np.array_equal(_bits(got[:lo]), _bits(base[:lo])) and np.array_equal(_bits(got[hi:]), _bits(base[hi:])), what
        mine, good = got[lo:hi], base[lo:hi]
        if kept_from is None:
            assert np.array_equal(_bits(mine), _bits(good)), what
        else:
            assert (mine[kept_from:] == canary).all(), what
            assert np.array_equal(_bits(mine[:kept_from]), _bits(good[:kept_from])), what


@pytest.mark.parametrize("with_gains", [False, True], ids=["keep", "follow"])
def test_merge_kernel_skips_a_device_row_outside_the_totals(with_gains):
    """The device rule of resample_merge_kernel (band_merge_why): the host table is correct, the DEVICE table differs from it in
    one field of one clip.  The clips are those of tests/test_band_host_cpu.py (513, 4097 and 9001 frames at 14 -> 48 kHz: one, two
    and three tiles).  Every buffer has 16 elements more than the table sums, and each altered row is checked, on the host, to lie
    inside what is allocated: a kernel that followed it would write wrong values, not fault.  The call succeeds; every output of
    the altered clip keeps the canary or, where the field does not reach its tile, has the bits of the unaltered call; every
    other clip has those bits throughout.  Without gains the two gains columns are not read at all.
    The bound n <= max_n (the outputs the time register describes) is reached alone only by a clip whose a covers more than the
    largest n and which is not the last in x: the second batch puts the 9001 frames in the middle, where 2626 samples of a cover
    9003 frames, and asks for 9002."""
    from sos_amd import _lib as L

    def cases(tab, n, m, mp, J, totals):
        tx, ta, tb, tg = totals
        return [("n: a does not cover it", 1, 1, 4098, 0),
                ("m: a leaves its total by one", 3, 1, ta - int(tab[2, 1]) + 1, 0), ("m = 0", 3, 1, 0, 0),
                ("m' above m", 5, 1, int(m[1]) + 1, 0), ("m' = 0", 5, 1, 0, 0),
                ("x offset: leaves the total by one", 0, 1, tx - int(n[1]) + 1, 0),
                ("a offset: leaves the total by one", 2, 1, ta - int(m[1]) + 1, 0),
                ("b offset: leaves the total by one", 4, 1, tb - int(mp[1]) + 1, 0),
                ("tile0: the clip starts a tile late", 8, 2, 4, 2 * L.RESAMPLE_CHUNK),     # tiles 4, 5 are its outputs 0 .. 8191
                ("J: one gain more", 7, 1, int(J[1]) + 1, 0 if with_gains else None),
                ("gains offset: leaves the total by one", 6, 1, tg - int(J[1]) + 1, 0 if with_gains else None)]

    def past_the_register(tab, n, m, mp, J, totals):
        # nothing but n > max_n refuses 9002: it stays inside x, a covers it, and no other column changed
        assert int(n.max()) == 9001 and int(tab[0, 1]) + 9002 <= totals[0] and int(float(m[1]) * (48000.0 / SR)) >= 9002
        return [("n: past the time register", 1, 1, 9002, 0)]

    _altered_device_rows(with_gains, [513, 4097, 9001], [100, 1106, 2528], cases)
    _altered_device_rows(with_gains, [513, 9001, 4097], [100, 2528, 1106], past_the_register)


# ---------------------------------------------------------------------------------------------- gains
def _gain_clips():
    """(a, b) pairs: a long clip whose m' leaves a partial last frame, with a run of silent input frames and a run of silenced
    output frames; a clip without any output (m' = 0); a clip of one partial frame (J = 1); a clip of whole frames with m' = m."""
    rng = np.random.default_rng(11)
    a0 = rng.standard_normal(2626).astype(np.float32)
    b0 = (0.6 * a0[:2528] + 0.2 * rng.standard_normal(2528)).astype(np.float32)
    a0[2 * HOP:9 * HOP] = 0.0                                    # E_a == 0 on frames 2 .. 8
    b0[9 * HOP:16 * HOP] = 0.0                                   # b silent on frames 9 .. 15, and frame 16 has no b at all
    a1 = rng.standard_normal(1195).astype(np.float32)
    a2 = rng.standard_normal(150).astype(np.float32)
    a3 = rng.standard_normal(5 * HOP).astype(np.float32)
    return [(a0, b0), (a1, np.zeros(0, np.float32)), (a2, 2.0 * a2[:100]), (a3, (0.5 * a3).astype(np.float32))]


@pytest.mark.parametrize("smooth", [0, 2, 16])
def test_gains_are_the_reference_within_one_rounding(smooth):
    from sos_amd import audio_io
    clips = _gain_clips()
    got = audio_io.band_gains_batch_device([_cuda(a) for a, _ in clips], [_cuda(b) for _, b in clips], HOP, smooth)
    assert [tuple(g.shape) for g in got] == [(17,), (8,), (1,), (5,)] and got[1].data_ptr() == got[0].data_ptr() + 4 * 17
    got = [g.cpu().numpy() for g in got]
    for (a, b), g in zip(clips, got):
        ref = B.gains(a, b, HOP, smooth)
        print(smooth, len(a), len(b), "max error", float(np.max(np.abs(g.astype(np.float64) - ref))))
        assert g.dtype == np.float32 and np.all(np.abs(g.astype(np.float64) - ref) <= 4 * 2.0 ** -24)
    assert np.all(got[1] == 0.0)                                 # no output at all: exactly 0
    if smooth == 0:
        assert np.all(got[0][2:9] == 1.0) and np.all(got[0][9:17] == 0.0)
        assert got[2][0] == 1.0                                  # more energy out than in: clipped to exactly 1
    if smooth == 2:                                              # windows that lie inside one run
        assert np.all(got[0][4:7] == 1.0) and np.all(got[0][11:15] == 0.0)
    alone = audio_io.band_gains_batch_device([_cuda(clips[0][0])], [_cuda(clips[0][1])], HOP, smooth)[0].cpu().numpy()
    assert np.all(np.abs(alone.astype(np.float64) - got[0]) <= 2.0 ** -24)


# ---------------------------------------------------------------------------------------------- end to end
# name, rate, channels, format, seconds; a 12 kHz tone of amplitude 0.1 is added to channel 0 of the 48 kHz file
SPECS = (("a", 48000, 2, "s16", 2.5), ("b", 44100, 1, "f32", 2.5), ("c", 14000, 1, "s16", 2.5), ("d", 8000, 1, "u8", 3.0))
TONE, AMP = 12000.0, 0.1


@pytest.fixture(autouse=True)
def _parity_mode():
    import sos_amd
    sos_amd.set_precision("bf16x3")
    try:
        yield
    finally:
        sos_amd.set_precision("bf16")


@pytest.fixture(scope="module")
def nets():
    from sos_amd.common import MyConfig
    from sos_amd.denoiser import networks as jnet
    from sos_amd.detector import networks as dnet
    det = dnet.get_network()
    det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    return det.cuda().eval(), jm.cuda().eval()


def _write(root, name, rate, ch, fmt, seconds, seed):
    n = int(round(seconds * rate))
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    planes = np.stack([0.3 * np.sin(2 * np.pi * (300 + 70 * c) * t) * (0.2 + (np.sin(2 * np.pi * 1.3 * t + c) > -0.4))
                       + 0.02 * rng.standard_normal(n) for c in range(ch)])
    if name == "a":
        planes[0] += AMP * np.sin(2 * np.pi * TONE * t)
    data, _ = R.encode(planes.astype(np.float32), fmt)
    path = root / (name + ".wav")
    path.write_bytes(R.container(data, fmt, ch, rate))
    return dict(name=name, path=str(path), rate=rate, channels=ch, fmt=fmt, frames=n, data=data)


def _amplitude(y, rate):
    t = np.arange(len(y)) / rate
    basis = np.stack([np.sin(2 * np.pi * TONE * t), np.cos(2 * np.pi * TONE * t)], axis=1)
    c, *_ = np.linalg.lstsq(basis, np.asarray(y, dtype=np.float64), rcond=None)
    return float(np.hypot(*c))


def _compose(nets, files):
    """The public pieces in denoise_recordings' order for one group: reference decode, resample_batch_device to 14 kHz per rate,
    ONE denoise_long, then per rate above 14 kHz the two new primitives and per rate below it resample_batch_device back.
    -> {mode: {name: (channels, n) planes on the host, before the encode}} for 'keep' and 'follow'."""
    from sos_amd import audio_io, windows
    owner = [f for f in files for _ in range(f["channels"])]
    natives = [_cuda(row) for f in files for row in R.decode(R.unpack(f["data"], f["fmt"], f["channels"]), f["fmt"])]
    clips = list(natives)
    rates = sorted({f["rate"] for f in files} - {SR})
    for rate in rates:
        idx = [k for k, f in enumerate(owner) if f["rate"] == rate]
        for k, y in zip(idx, audio_io.resample_batch_device([natives[k] for k in idx], rate, SR)):
            clips[k] = y
    lows = windows.denoise_long(nets[0], nets[1], clips, **SECONDS)
    out = {}
    for mode in ("keep", "follow"):
        outs = list(lows)
        for rate in rates:
            idx = [k for k, f in enumerate(owner) if f["rate"] == rate]
            a, b = [clips[k] for k in idx], [lows[k] for k in idx]
            if rate > SR:
                gains = audio_io.band_gains_batch_device(a, b, HOP, 2) if mode == "follow" else None
                back = audio_io.resample_merge_batch_device([natives[k] for k in idx], a, b, SR, rate, gains)
            else:
                back = audio_io.resample_batch_device(b, SR, rate)
            for k, y in zip(idx, back):
                outs[k] = y
        out[mode], k = {}, 0
        for f in files:
            out[mode][f["name"]] = np.stack([o.cpu().numpy() for o in outs[k:k + f["channels"]]])
            k += f["channels"]
    return out


@pytest.fixture(scope="module")
def runs(nets, tmp_path_factory):
    """denoise_recordings over the four files as one group without the argument and under each mode, the composition, and the
    48 kHz file alone written as f32 under 'drop' and 'keep': computed once and left unchanged."""
    import sos_amd
    from sos_amd import recordings
    root = tmp_path_factory.mktemp("band_in")
    files = [_write(root, *spec, seed=71 + i) for i, spec in enumerate(SPECS)]
    paths = [f["path"] for f in files]
    sos_amd.set_precision("bf16x3")
    try:
        res = dict(default=recordings.denoise_recordings(nets[0], nets[1], paths, str(tmp_path_factory.mktemp("band_default")), **SECONDS))
        for mode in ("drop", "keep", "follow"):
            res[mode] = recordings.denoise_recordings(nets[0], nets[1], paths, str(tmp_path_factory.mktemp("band_" + mode)),
                                                      high_band=mode, **SECONDS)
        planes = _compose(nets, files)
        f32 = {mode: recordings.denoise_recordings(nets[0], nets[1], paths[:1], str(tmp_path_factory.mktemp("band_f32_" + mode)),
                                                   sample_format="f32", high_band=mode, **SECONDS) for mode in ("drop", "keep")}
    finally:
        sos_amd.set_precision("bf16")
    return dict(files=files, res=res, planes=planes, f32=f32)


def _read(path):
    with open(path, "rb") as fp:
        return fp.read()


@pytest.mark.parametrize("mode", ["keep", "follow"])
def test_written_bytes_are_the_composition_of_public_pieces(runs, mode):
    from sos_amd import audio_io
    for f, r in zip(runs["files"], runs["res"][mode]):
        data, clipped = R.encode(runs["planes"][mode][f["name"]], f["fmt"], f["frames"])
        assert _read(r["out_path"]) == R.container(data, f["fmt"], f["channels"], f["rate"]), f["name"]
        assert r["clipped"] == clipped
        tag, bits = R.TAG_BITS[f["fmt"]]
        assert audio_io.wave_info(r["out_path"]) == dict(tag=tag, bits=bits, channels=f["channels"], rate=f["rate"], frames=f["frames"])
        assert set(r) == {"path", "out_path", "channels", "rate", "frames", "format", "clipped", "windows"}


def test_drop_is_the_call_without_the_argument_and_low_rates_do_not_depend_on_the_mode(runs):
    res = runs["res"]
    for i, f in enumerate(runs["files"]):
        want = _read(res["default"][i]["out_path"])
        assert _read(res["drop"][i]["out_path"]) == want, f["name"]
        same = [_read(res[mode][i]["out_path"]) == want for mode in ("keep", "follow")]
        assert same == ([True, True] if f["rate"] <= SR else [False, False]), (f["name"], same)
        for mode in ("drop", "keep", "follow"):
            assert {k: v for k, v in res[mode][i].items() if k not in ("out_path", "clipped")} == \
                   {k: v for k, v in res["default"][i].items() if k not in ("out_path", "clipped")}


def test_keep_returns_the_12_khz_tone_that_the_14_khz_chain_removes(runs):
    """The user-visible defect: the source holds a 12 kHz tone of amplitude 0.1; the default output has lost it.  keep - drop is
    x - U(a), whatever the networks did, so its 12 kHz component is the source's."""
    f = runs["files"][0]
    src = R.decode(R.unpack(f["data"], f["fmt"], f["channels"]), f["fmt"])[0]
    out = {}
    for mode in ("drop", "keep"):
        blob = _read(runs["f32"][mode][0]["out_path"])
        at = blob.index(b"data") + 8
        out[mode] = np.frombuffer(blob[at:], dtype="<f4").reshape(-1, f["channels"])[:, 0]
        assert len(out[mode]) == f["frames"]
    a_src, a_drop, a_keep = _amplitude(src, f["rate"]), _amplitude(out["drop"], f["rate"]), _amplitude(out["keep"], f["rate"])
    a_diff = _amplitude(out["keep"].astype(np.float64) - out["drop"], f["rate"])
    print("12 kHz amplitude: source %.5f, drop %.3g, keep %.5f, keep - drop %.5f" % (a_src, a_drop, a_keep, a_diff))
    assert abs(a_src - AMP) < 0.02 * AMP
    assert abs(a_diff - a_src) <= 0.02 * a_src
    assert a_drop < 0.01 * a_src                                 # what 'drop' leaves of it
