"""The batched wave front door (sos_resample_batch_f32, audio_io.resample_batch_device / load_batch_device): a ragged batch
of clips resampled in one launch gives every clip, bit for bit, what the one-clip call gives it -- alone, in any batch, in
any order -- and stays within the one-clip tolerance of the oracle (oracle/wave_io.py).

The clip lengths are the smallest at which the kernel can go wrong: the shortest legal clips, clips shorter than the filter's
2 x 202 taps (both wings cut by the clip's own ends), lone zero-padding samples past a 4096-output tile boundary, clips that
end exactly on one, and several-tile clips.  Every second clip is 1e3 times louder than its neighbours, so a tap that reads a
neighbour's samples in the concatenated buffer is an error hundreds of times the quiet clip's peak."""
import numpy as np
import pytest
import scipy.io.wavfile
import torch

from oracle import wave_io as owio
from test_gpu_metrics_batch import _sync_warnings
from test_gpu_wave_io import RESAMPLE_TOL, peak_err

pytestmark = pytest.mark.gpu

# (orig_sr, target_sr): [(clip length, n_valid, n_out)]
CASES = {
    (44100, 14000): [(4, 1, 2), (700, 222, 223), (12903, 4096, 4097), (12905, 4096, 4097), (50001, 15873, 15874)],
    (14000, 16000): [(1, 1, 2), (2, 2, 3), (7, 8, 8), (130, 148, 149), (3584, 4096, 4096), (3585, 4097, 4098),
                     (14001, 16001, 16002), (28000, 32000, 32000), (33333, 38094, 38095)],
    (48000, 14000): [(14044, 4096, 4097), (20000, 5833, 5834)],
}
_cache = {}


def _clips(rates):
    """Seeded standard-normal clips of the case's lengths (every second one scaled by 1e3) and their oracle resamplings,
    computed once per rate pair and never modified."""
    if rates not in _cache:
        rng = np.random.default_rng(sum(rates))
        xs = [(rng.standard_normal(n) * (1e3 if i % 2 else 1.0)).astype(np.float32) for i, (n, _, _) in enumerate(CASES[rates])]
        refs = [owio.resample(x, *rates) for x in xs]
        for a in xs + refs:
            a.setflags(write=False)
        _cache[rates] = (xs, refs)
    return _cache[rates]


@pytest.mark.parametrize("rates", list(CASES), ids=["44k1-14k", "14k-16k", "48k-14k"])
def test_batch_equals_the_one_clip_call_and_the_oracle(rates):
    from sos_amd import audio_io
    xs, refs = _clips(rates)
    dev = [torch.from_numpy(x).cuda() for x in xs]
    one = [audio_io.resample_device(d, *rates) for d in dev]
    got = audio_io.resample_batch_device(dev, *rates)
    assert isinstance(got, list) and len(got) == len(xs)
    for i, ((n, n_valid, n_out), g, o, ref) in enumerate(zip(CASES[rates], got, one, refs)):
        assert g.dtype == torch.float32 and g.dim() == 1 and g.is_cuda
        assert g.numel() == n_out == ref.shape[0] == int(np.ceil(n * rates[1] / rates[0])), (i, n)
        assert n_valid == min(int(n * (float(rates[1]) / rates[0])), n_out)
        assert torch.equal(g, o), f"clip {i} (n={n}) differs from resample_device"
        err = peak_err(g.cpu().numpy(), ref)
        print(f"{rates} clip {i} n={n}: {err:.3g} of the peak against the oracle")
        assert err < RESAMPLE_TOL, (i, n, err)
    rev = audio_io.resample_batch_device(dev[::-1], *rates)[::-1]
    for i, (g, r, d) in enumerate(zip(got, rev, dev)):
        assert torch.equal(g, r), f"clip {i}: the reversed batch gives other bits"
        alone = audio_io.resample_batch_device([d], *rates)
        assert len(alone) == 1 and torch.equal(alone[0], g), f"clip {i}: a batch of one gives other bits"
    floor = audio_io.resample_batch_device(dev, *rates, fix=False)
    for (n, n_valid, _), f, g in zip(CASES[rates], floor, got):
        assert f.numel() == n_valid == int(n * (float(rates[1]) / rates[0])) and torch.equal(f, g[:n_valid])
    host = audio_io.resample_batch(xs, *rates)
    assert all(h.dtype == np.float32 and np.array_equal(h, g.cpu().numpy()) for h, g in zip(host, got))
    scaled = audio_io.resample_batch(xs[:2], *rates, scale=True)
    assert all(np.array_equal(s, audio_io.resample(x, *rates, scale=True)) for s, x in zip(scaled, xs))


def _many():
    rng = np.random.default_rng(301)
    lens = [int(n) for n in rng.integers(1, 41, size=300)]
    lens.insert(150, 9000)
    return [torch.from_numpy((rng.standard_normal(n) * (1e3 if i % 2 else 1.0)).astype(np.float32)).cuda()
            for i, n in enumerate(lens)]


def test_many_short_clips_and_the_clip_cap(monkeypatch):
    """301 clips: the tile table over hundreds of one-tile clips and one three-tile clip; then the same with the cap on
    clips per launch set to 7, so that the batch is cut into 43 launches at clip boundaries."""
    from sos_amd import audio_io
    dev = _many()
    one = [audio_io.resample_device(d, 14000, 16000) for d in dev]
    got = audio_io.resample_batch_device(dev, 14000, 16000)
    assert len(got) == 301
    for i, (g, o) in enumerate(zip(got, one)):
        assert torch.equal(g, o), f"clip {i} (n={dev[i].numel()})"
    monkeypatch.setattr("sos_amd.ragged.MAX_CLIPS", 7)
    cut = audio_io.resample_batch_device(dev, 14000, 16000)
    for i, (g, o) in enumerate(zip(cut, one)):
        assert torch.equal(g, o), f"clip {i} (n={dev[i].numel()}) with 7 clips per launch"


def test_kernel_skips_a_device_entry_outside_the_totals():
    """The device rule of resample_batch_kernel: the host table is correct, the DEVICE table differs in one entry of clip 1 (its
    input one sample past the total; more resampled outputs than outputs).  Every buffer has 16 spare elements, so an entry that
    is wrongly followed touches allocated memory only.  The call succeeds, clip 1's outputs stay as they were and every other
    clip gets the bits of the unaltered call."""
    import ctypes as C
    from sos_amd import _lib as L
    from sos_amd import audio_io
    spare, sentinel, ratio = 16, -77.0, 16000 / 14000
    n_in = np.asarray([7, 130, 2, 300], dtype=np.int64)
    n_out = np.asarray([int(np.ceil(int(n) * ratio)) for n in n_in], dtype=np.int64)
    n_valid = np.minimum(np.asarray([int(int(n) * ratio) for n in n_in], dtype=np.int64), n_out)
    tiles = -(-n_out // L.RESAMPLE_CHUNK)
    tab = np.ascontiguousarray(np.stack([np.cumsum(n_in) - n_in, n_in, np.cumsum(n_out) - n_out, n_out, n_valid,
                                         np.cumsum(tiles) - tiles]), dtype=np.int64)
    total_in, total_out = int(n_in.sum()), int(n_out.sum())
    x = torch.from_numpy(np.random.default_rng(5).standard_normal(total_in + spare).astype(np.float32)).cuda()
    win, num_table = audio_io._filter_on(x.device, ratio, "kaiser_best")

    def run(d_tab):
        out = torch.full((total_out + spare,), sentinel, device="cuda")
        rc = L.lib().sos_resample_batch_f32(L.ptr(x), L.ptr(d_tab), tab.ctypes.data_as(C.c_void_p), len(n_in), ratio, L.ptr(win),
                                            win.numel(), num_table, L.ptr(out), L.stream_ptr())
        return rc, out.cpu().numpy()

    rc, base = run(torch.from_numpy(tab).cuda())
    assert rc == 0 and not (base[:total_out] == sentinel).any() and (base[total_out:] == sentinel).all()
    lo, hi = int(tab[2, 1]), int(tab[2, 1] + n_out[1])
    for what, row, value in (("input offset", 0, total_in - int(n_in[1]) + 1), ("n_valid", 4, int(n_out[1]) + 1)):
        d_tab = torch.from_numpy(tab).cuda()
        d_tab[row, 1] = value
        rc, got = run(d_tab)
        assert rc == 0, what
        assert (got[lo:hi] == sentinel).all() and (got[total_out:] == sentinel).all(), what
        assert np.array_equal(got[:lo].view(np.uint32), base[:lo].view(np.uint32)), what
        assert np.array_equal(got[hi:total_out].view(np.uint32), base[hi:total_out].view(np.uint32)), what


def test_errors_and_trivial_cases():
    from sos_amd import audio_io
    xs, _ = _clips((44100, 14000))
    dev = [torch.from_numpy(x).cuda() for x in xs]
    with pytest.raises(ValueError, match=r"clip 2\b.*length=3 is too small"):
        audio_io.resample_batch_device(dev[:2] + [dev[1][:3]] + dev[2:], 44100, 14000)
    with pytest.raises(RuntimeError):
        audio_io.resample_batch_device([dev[0], torch.from_numpy(xs[1])], 44100, 14000)     # host tensor: no CPU fallback
    with pytest.raises(ValueError):
        audio_io.resample_batch_device(dev, 44100, 14000, res_type="kaiser_fast")
    with pytest.raises(ValueError):
        audio_io.resample_batch(xs, 44100, 14000, res_type="kaiser_fast")
    same = audio_io.resample_batch_device(dev, 14000, 14000)
    assert len(same) == len(dev) and all(a is b for a, b in zip(same, dev))
    assert audio_io.resample_batch_device([], 44100, 14000) == []
    assert audio_io.resample_batch([], 44100, 14000) == []


def test_host_waits_do_not_grow_with_the_batch():
    """resample_batch_device waits for the device the same number of times (the table upload) for 8 and for 64 clips.  The
    loop it replaces at the file level, resample() per clip (one upload and one download each), grows with the clips."""
    from sos_amd import audio_io
    rng = np.random.default_rng(64)
    xs = [rng.standard_normal(1000 + 37 * i).astype(np.float32) for i in range(64)]
    dev = [torch.from_numpy(x).cuda() for x in xs]
    audio_io.resample_batch_device(dev[:2], 14000, 16000)          # warm-up: code object and filter table
    w8 = _sync_warnings(lambda: audio_io.resample_batch_device(dev[:8], 14000, 16000))
    w64 = _sync_warnings(lambda: audio_io.resample_batch_device(dev, 14000, 16000))
    h8 = _sync_warnings(lambda: audio_io.resample_batch(xs[:8], 14000, 16000))
    h64 = _sync_warnings(lambda: audio_io.resample_batch(xs, 14000, 16000))
    loop2 = _sync_warnings(lambda: [audio_io.resample(x, 14000, 16000) for x in xs[:2]])
    loop4 = _sync_warnings(lambda: [audio_io.resample(x, 14000, 16000) for x in xs[:4]])
    print(f"synchronisation warnings: device batch of 8: {w8}, of 64: {w64}; host batch of 8: {h8}, of 64: {h64}; "
          f"loop over 2 clips: {loop2}, over 4: {loop4}")
    assert w8 == w64 and h8 == h64
    assert loop4 > loop2 > 0                                       # the counter counts, and the loop grows with the clips


def _write_files(tmp_path):
    rng = np.random.default_rng(77)
    spec = [("a_44k_stereo_s16", 44100, 2, np.int16, 0.45), ("b_44k_mono_s16", 44100, 1, np.int16, 0.37),
            ("c_48k_stereo_f32", 48000, 2, np.float32, 0.41), ("d_14k_mono_s16", 14000, 1, np.int16, 0.5),
            ("e_44k_stereo_s16", 44100, 2, np.int16, 0.613)]
    paths = []
    for name, sr, ch, dtype, secs in spec:
        sig = 0.3 * rng.standard_normal((int(sr * secs), ch))
        pcm = np.clip(sig * 32768, -32768, 32767).astype(np.int16) if dtype == np.int16 else sig.astype(np.float32)
        paths.append(str(tmp_path / (name + ".wav")))
        scipy.io.wavfile.write(paths[-1], sr, pcm if ch > 1 else pcm[:, 0])
    return paths, [s[1] for s in spec]


def test_load_batch_equals_the_one_file_call(tmp_path):
    from sos_amd import audio_io
    paths, native = _write_files(tmp_path)
    ys, srs = audio_io.load_batch_device(paths, sr=14000)
    assert srs == [14000] * 5 and len(ys) == 5
    for p, y in zip(paths, ys):
        want, sr = audio_io.load_device(p, sr=14000)
        assert sr == 14000 and y.dtype == torch.float32 and y.is_cuda and torch.equal(y, want), p
    ys_n, srs_n = audio_io.load_batch_device(paths, sr=None)
    assert srs_n == native
    for p, y, r in zip(paths, ys_n, native):
        want, sr = audio_io.load_device(p, sr=None)
        assert sr == r and y.numel() > 0 and torch.equal(y, want), p
    ys_o, srs_o = audio_io.load_batch_device(paths, sr=14000, offset=0.1, duration=0.2)
    for p, y in zip(paths, ys_o):
        want, _ = audio_io.load_device(p, sr=14000, offset=0.1, duration=0.2)
        assert y.numel() == 2800 and torch.equal(y, want), p
    hs, hsr = audio_io.load_batch(paths, sr=14000)
    assert hsr == srs and all(isinstance(h, np.ndarray) and h.dtype == np.float32 and np.array_equal(h, y.cpu().numpy())
                              for h, y in zip(hs, ys))
    with pytest.raises(NotImplementedError):
        audio_io.load_batch_device(paths, sr=14000, mono=False)
    # an empty file gives an empty tensor, as load_device does, and leaves its neighbours alone
    ys_e, srs_e = audio_io.load_batch_device(paths, sr=14000, offset=0.45)
    for p, y in zip(paths, ys_e):
        want, _ = audio_io.load_device(p, sr=14000, offset=0.45)
        assert torch.equal(y, want), p
    assert ys_e[0].numel() == 0 and ys_e[1].numel() == 0 and ys_e[4].numel() > 0 and srs_e == [14000] * 5
