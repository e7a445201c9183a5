"""The launch sequences of planes.py, resampling.py and metrics.loudness_batch going round more than once: with ragged.MAX_CLIPS
set to 3 and 7 files or clips the chunks have 3, 3 and 1 rows, every array is re-based to its chunk's first element, and the last
chunk starts off any alignment.  Every result must be, bit for bit, that of the same call in one chunk -- the kernels see the
same clips either way, only through other tables and base pointers.  (resample_batch_device has this test in
test_gpu_wave_io_batch.py.)  Last in the file, on any machine: every public name of audio_io is the object of its new home."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
FILES = 7


def _chunked_and_whole(monkeypatch, call, chunks=3):
    """call() in one launch sequence and in chunks of 3: (whole, chunked), after checking that the chunked call uploaded `chunks`
    tables for every one of the whole call."""
    from sos_amd import ragged
    uploads = []
    staged = ragged.upload

    def counting(host, device):
        uploads.append(host.dtype == np.int64)
        return staged(host, device)

    with monkeypatch.context() as m:
        m.setattr("sos_amd.ragged.upload", counting)
        whole = call()
        tables = sum(uploads)
        m.setattr("sos_amd.ragged.MAX_CLIPS", 3)
        del uploads[:]
        chunked = call()
    assert tables >= 1 and sum(uploads) == chunks * tables, (tables, sum(uploads))
    torch.cuda.synchronize()
    return whole, chunked


def _planes(rng, amp=0.5):
    """7 files of 1 .. 3 channels and 5 .. 400 frames as (channels, n) float32 arrays."""
    shapes = [(1, 5), (2, 400), (3, 57), (1, 158), (2, 33), (3, 400), (2, 91)]
    return [(amp * rng.standard_normal(s)).astype(np.float32) for s in shapes]


@gpu
@pytest.mark.parametrize("kinds", [["s16"] * FILES, ["s16", "ulaw", "s16", "s16", "ulaw", "s16", "ulaw", "s16", "ulaw", "ulaw"]],
                         ids=["one-format", "two-formats-and-an-empty-file"])
def test_decode_planes_in_chunks(monkeypatch, kinds):
    from sos_amd import audio_io
    rng = np.random.default_rng(1)
    frames = [5, 400, 57, 0 if len(kinds) > FILES else 158, 33, 400, 91, 12, 7, 301][:len(kinds)]
    chans = [1, 2, 3, 1, 2, 3, 2, 1, 3, 2][:len(kinds)]
    arrs = [rng.integers(-32768, 32768, (n, c)).astype(np.int16) if k == "s16" else rng.integers(0, 256, (n, c)).astype(np.uint8)
            for k, n, c in zip(kinds, frames, chans)]
    if len(kinds) > FILES:                                      # four files of s16 with samples (3 + 1) and five of ulaw (3 + 2)
        assert sum(k == "s16" and n > 0 for k, n in zip(kinds, frames)) == 4 and kinds.count("ulaw") == 5 and not frames[3]
    go = lambda: audio_io.decode_planes_batch_device(arrs, kinds)                   # noqa: E731
    whole, chunked = _chunked_and_whole(monkeypatch, go, 2 if len(kinds) > FILES else 3)     # two formats: 2 chunks each
    assert len(whole) == len(chunked) == len(arrs)
    for w, c, a in zip(whole, chunked, arrs):
        assert c.shape == (a.shape[1], a.shape[0]) and torch.equal(w, c)
    for i in (0, 2, 5):                                         # and they are the samples: s16 / 2^15
        assert np.array_equal(chunked[i].cpu().numpy(), arrs[i].T.astype(np.float32) / 32768.0)


@gpu
@pytest.mark.parametrize("fmt", ["s16", "s24", "alaw"])
def test_encode_in_chunks(monkeypatch, fmt):
    """frames shorter and longer than the planes; 1.4 sigma of the samples saturate, so the counts are not all zero."""
    from sos_amd import audio_io
    host = _planes(np.random.default_rng(2), amp=0.7)
    frames = [p.shape[1] + d for p, d in zip(host, (3, -100, 0, 40, -33, 1, -1))]
    planes = [torch.from_numpy(p).cuda() for p in host]
    (data, offsets, clipped), (data3, offsets3, clipped3) = _chunked_and_whole(
        monkeypatch, lambda: audio_io.encode_batch_device(planes, fmt, frames=frames))
    width = {"s16": 2, "s24": 3, "alaw": 1}[fmt]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([width * p.shape[0] * f for p, f in zip(host, frames)])]).tolist()
    assert np.array_equal(offsets, offsets3) and offsets3.dtype == np.int64
    assert torch.equal(data, data3) and torch.equal(clipped, clipped3)
    assert int(clipped.sum()) > 0 and int(clipped[1]) > 0


def _band_clips(rng):
    """7 clips at 14 kHz -> 48 kHz: a of 300 .. 2000 samples, b shorter or as long, x of the frames a covers or a few less."""
    ratio = 48000.0 / 14000.0
    m = [300, 2000, 1023, 158, 1580, 477, 1999]
    mp = [300, 1896, 1, 158, 1422, 400, 1999]
    n = [int(k * ratio) - d for k, d in zip(m, (0, 3, 1, 0, 2, 0, 1))]
    f32 = lambda k: torch.from_numpy(rng.standard_normal(k).astype(np.float32)).cuda()         # noqa: E731
    a = [f32(k) for k in m]
    b = [0.5 * t[:k] + 0.01 * f32(k) for t, k in zip(a, mp)]
    return [f32(k) for k in n], a, b


@gpu
def test_band_gains_and_merge_in_chunks(monkeypatch):
    from sos_amd import audio_io
    x, a, b = _band_clips(np.random.default_rng(3))
    gains, gains3 = _chunked_and_whole(monkeypatch, lambda: audio_io.band_gains_batch_device(a, b))
    assert [g.numel() for g in gains3] == [-(-t.numel() // 158) for t in a]
    for g, g3 in zip(gains, gains3):
        assert torch.equal(g, g3)
    assert float(torch.cat(gains).min()) < 0.9                  # not all ones: the gains do weigh the band
    for s in (None, gains):
        out, out3 = _chunked_and_whole(monkeypatch, lambda: audio_io.resample_merge_batch_device(x, a, b, 14000, 48000, s))
        assert [t.numel() for t in out3] == [t.numel() for t in x]
        for y, y3 in zip(out, out3):
            assert torch.equal(y, y3)
    keep = audio_io.resample_merge_batch_device(x, a, b, 14000, 48000)
    assert not torch.equal(torch.cat(keep), torch.cat(out3))


@gpu
def test_loudness_and_gain_in_chunks(monkeypatch):
    """Rates and lengths of the first seven files of test_gpu_loudness.py's batch: 8000 Hz (h = 800) with 4h - 1 (no block), 4h,
    5h - 1, 5h and 3 s + 17 samples, 11025 Hz (h = 1103) with 4h - 1 and 4h; 1 .. 3 channels; one file zero-filled past its plane
    and one cropped."""
    from sos_amd import audio_io, metrics
    rng = np.random.default_rng(4)
    rates = [8000] * 5 + [11025] * 2
    lengths = [3199, 3200, 3999, 4000, 24017, 4411, 4412]
    chans = [1, 2, 3, 1, 2, 2, 3]
    frames = [3199, 3200, 3999 + 801, 4000, 24017 - 1000, 4411, 4412]
    host = [(0.1 * (1 + i) * rng.standard_normal((c, n))).astype(np.float32) for i, (c, n) in enumerate(zip(chans, lengths))]
    weights = [None, [1.0, 0.5], None, None, None, None, [1.0, 1.0, 1.41]]

    def go():
        planes = [torch.from_numpy(p).cuda() for p in host]                        # the gain works in place: fresh planes per call
        rows = metrics.loudness_batch(planes, rates, weights, frames)["rows"]
        gains, limited = audio_io.loudness_gain_batch_device(planes, rows, -23.0, -1.0, frames=frames)
        return rows, gains, limited, planes

    (rows, gains, limited, planes), (rows3, gains3, limited3, planes3) = _chunked_and_whole(monkeypatch, go)
    assert torch.equal(rows, rows3) and torch.equal(gains, gains3) and torch.equal(limited, limited3)
    for p, p3 in zip(planes, planes3):
        assert torch.equal(p, p3)
    got = rows3.cpu().numpy()
    assert got[0, 0] == -np.inf and got[5, 0] == -np.inf and np.all(np.isfinite(got[[1, 2, 3, 4, 6], 0])) and np.all(got[:, 1] > 0)
    g = gains3.cpu().numpy()
    assert g[0] == 1.0 and g[5] == 1.0 and np.all(g[[1, 2, 3, 4, 6]] != 1.0)
    assert not torch.equal(planes3[4], torch.from_numpy(host[4]).cuda()) and torch.equal(planes3[4][:, frames[4]:], torch.from_numpy(host[4][:, frames[4]:]).cuda())


# every public name of audio_io before it was split by layer, and where it lives now
HOMES = {
    "wave_file": ["WaveFormatError", "read_wave", "read_wave_info", "wave_info", "file_groups", "wave_bytes", "wave_container", "write_wav",
                  "ENCODINGS", "G711"],
    "resampling": ["KAISER_BEST", "sinc_window", "resample_device", "resample_batch_device", "band_gains_batch_device",
                   "resample_merge_batch_device"],
    "planes": ["pcm_to_mono_device", "decode_planes_batch_device", "load_channels_batch_device", "encode_batch_device", "planes_of",
               "planes_together", "loudness_gain_batch_device", "g711_decode_device", "g711_encode_device"],
    "stream_resampling": ["StreamResampler", "StreamBandMerger"],
    "audio_io": ["load", "load_device", "load_batch", "load_batch_device", "resample", "resample_batch", "to_mono"],
}


def test_every_public_name_of_audio_io_is_its_new_home_s():
    import importlib
    from sos_amd import audio_io, stream
    assert sum(len(v) for v in HOMES.values()) == 34
    for home, names in HOMES.items():
        module = importlib.import_module("sos_amd." + home)
        for name in names:
            assert getattr(audio_io, name) is getattr(module, name), name
            if callable(getattr(module, name)):
                assert getattr(module, name).__module__.endswith("." + home), name
    assert stream.StreamResampler is audio_io.StreamResampler and stream.StreamBandMerger is audio_io.StreamBandMerger
    # the two private names the older tests read are views of the new homes, not second statements
    assert audio_io._filter_on is audio_io.filter_on
    assert audio_io._FMT == {k: c for k, (family, c) in audio_io.DECODE.items() if family == "pcm"} == {"s16": 0, "s32": 1, "f32": 2, "u8": 3}
