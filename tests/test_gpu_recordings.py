"""recordings.denoise_recordings end to end: WAVE files of four rates, channel counts and sample formats in, files of the same
frame count, channels, rate and format out.  bf16x3, the closed-form networks of the hand-off tests.  The bound is equality: the
written bytes are those of the composition of public pieces in the same order -- reference decode (tests/pcm_reference.py),
resample_batch_device to 14 kHz, ONE denoise_long over all channels in file-and-channel order, resample_batch_device back,
reference encode with the source's frame count -- for the same grouping of files (denoise_long's batches differ by composition,
so another grouping is only asked for valid files of the right shape)."""
import os

import numpy as np
import pytest
import torch

import pcm_reference as R
from oracle import nets as onet

pytestmark = pytest.mark.gpu
SECONDS = dict(window_seconds=2.0, context_seconds=0.5)
# name, rate, channels, format, seconds: the 5 s file runs in two windows per channel
SPECS = (("a", 44100, 2, "s16", 2.5), ("b", 14000, 1, "f32", 2.5), ("c", 48000, 3, "s24", 5.0), ("d", 8000, 1, "u8", 3.0))
WINDOWS = dict(a=2, b=1, c=6, d=1)


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
                       + 0.02 * rng.standard_normal(n) for c in range(ch)]).astype(np.float32)
    data, _ = R.encode(planes, fmt)
    path = root / (name + ".wav")
    path.write_bytes(R.container(data, fmt, ch, rate))
    return dict(name=name, path=str(path), rate=rate, channels=ch, fmt=fmt, frames=n, data=data)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("recordings_in")
    return [_write(root, *spec, seed=53 + i) for i, spec in enumerate(SPECS)]


def _compose(nets, files, groups):
    """The public pieces in denoise_recordings' order, per group of files: -> per file the (channels, n) planes at its own rate,
    on the host, before the encode."""
    from sos_amd import audio_io, pipeline, windows
    out = {}
    for group in groups:
        fs = [files[i] for i in group]
        owner = [f for f in fs for _ in range(f["channels"])]
        clips = [torch.from_numpy(np.ascontiguousarray(row)).cuda() for f in fs
                 for row in R.decode(R.unpack(f["data"], f["fmt"], f["channels"]), f["fmt"])]
        for rate in sorted({f["rate"] for f in fs} - {pipeline.SR}):
            idx = [k for k, f in enumerate(owner) if f["rate"] == rate]
            for k, y in zip(idx, audio_io.resample_batch_device([clips[k] for k in idx], rate, pipeline.SR)):
                clips[k] = y
        outs = windows.denoise_long(nets[0], nets[1], clips, **SECONDS)
        for rate in sorted({f["rate"] for f in fs} - {pipeline.SR}):
            idx = [k for k, f in enumerate(owner) if f["rate"] == rate]
            for k, y in zip(idx, audio_io.resample_batch_device([outs[k] for k in idx], pipeline.SR, rate)):
                outs[k] = y
        k = 0
        for f in fs:
            out[f["name"]] = np.stack([o.cpu().numpy() for o in outs[k:k + f["channels"]]])
            k += f["channels"]
    return out


@pytest.fixture(scope="module")
def one_group(nets, files, tmp_path_factory):
    """denoise_recordings over the four files as one group, and the composition: computed once and left unchanged."""
    import sos_amd
    from sos_amd import recordings
    out_dir = tmp_path_factory.mktemp("recordings_out")
    sos_amd.set_precision("bf16x3")
    try:
        res = recordings.denoise_recordings(nets[0], nets[1], [f["path"] for f in files], str(out_dir), suffix="_dn", **SECONDS)
        planes = _compose(nets, files, [[0, 1, 2, 3]])
    finally:
        sos_amd.set_precision("bf16")
    return res, planes


def _check_shape(f, out_path):
    from sos_amd import audio_io
    tag, bits = R.TAG_BITS[f["fmt"]]
    assert audio_io.wave_info(out_path) == dict(tag=tag, bits=bits, channels=f["channels"], rate=f["rate"], frames=f["frames"])


def test_written_files_keep_tag_bits_channels_rate_and_frames(one_group, files):
    res, _ = one_group
    assert [r["path"] for r in res] == [f["path"] for f in files]
    for f, r in zip(files, res):
        assert os.path.basename(r["out_path"]) == f["name"] + "_dn.wav"
        _check_shape(f, r["out_path"])
        assert (r["channels"], r["rate"], r["frames"], r["format"]) == (f["channels"], f["rate"], f["frames"], f["fmt"])
        assert r["windows"] == WINDOWS[f["name"]]
        assert set(r) == {"path", "out_path", "channels", "rate", "frames", "format", "clipped", "windows"}


def test_written_bytes_and_counts_are_the_composition_of_public_pieces(one_group, files):
    res, planes = one_group
    for f, r in zip(files, res):
        p = planes[f["name"]]
        assert p.shape[0] == f["channels"]
        data, clipped = R.encode(p, f["fmt"], f["frames"])
        print(f["name"], "planes", p.shape, "frames", f["frames"], "clipped", r["clipped"], "reference", clipped)
        with open(r["out_path"], "rb") as fp:
            assert fp.read() == R.container(data, f["fmt"], f["channels"], f["rate"]), f["name"]
        assert r["clipped"] == clipped


def test_two_groups_write_valid_files_equal_to_the_same_grouping(nets, files, tmp_path):
    from sos_amd import recordings
    res = recordings.denoise_recordings(nets[0], nets[1], [f["path"] for f in files], str(tmp_path), max_bytes=3100000, **SECONDS)
    planes = _compose(nets, files, [[0, 1], [2, 3]])            # 882 000 + 140 000 bytes, then 2 880 000 + 96 000
    for f, r in zip(files, res):
        _check_shape(f, r["out_path"])
        data, clipped = R.encode(planes[f["name"]], f["fmt"], f["frames"])
        with open(r["out_path"], "rb") as fp:
            assert fp.read() == R.container(data, f["fmt"], f["channels"], f["rate"]), f["name"]
        assert r["clipped"] == clipped


def test_sample_format_forces_one_format_for_all_files(one_group, nets, files, tmp_path):
    from sos_amd import audio_io, recordings
    _, planes = one_group
    res = recordings.denoise_recordings(nets[0], nets[1], [f["path"] for f in files], str(tmp_path), sample_format="s16", **SECONDS)
    for f, r in zip(files, res):
        assert r["format"] == "s16"
        assert audio_io.wave_info(r["out_path"]) == dict(tag=1, bits=16, channels=f["channels"], rate=f["rate"], frames=f["frames"])
        data, clipped = R.encode(planes[f["name"]], "s16", f["frames"])
        with open(r["out_path"], "rb") as fp:
            assert fp.read() == R.container(data, "s16", f["channels"], f["rate"]), f["name"]
        assert r["clipped"] == clipped


def test_a_file_too_short_for_the_networks_is_named_and_nothing_is_written(nets, files, tmp_path):
    """MIN_FRAMES = 65 STFT frames of hop 158 are 0.73 s at 14 kHz: a 0.5 s file is below that at any rate."""
    from sos_amd import recordings
    short = _write(tmp_path, "short", 44100, 2, "s16", 0.5, seed=3)
    out_dir = tmp_path / "out"
    with pytest.raises(ValueError, match="short.wav"):
        recordings.denoise_recordings(nets[0], nets[1], [files[1]["path"], short["path"]], str(out_dir), **SECONDS)
    assert not out_dir.exists() or not os.listdir(out_dir)
    with pytest.raises(ValueError, match="sample_format"):
        recordings.denoise_recordings(nets[0], nets[1], [files[1]["path"]], str(out_dir), sample_format="s12", **SECONDS)
    bad = tmp_path / "adpcm.wav"
    bad.write_bytes(R.container(b"\0" * 64, "s16", 1, 8000).replace(b"\x01\x00\x01\x00", b"\x02\x00\x01\x00", 1))   # tag 2
    with pytest.raises(ValueError, match="adpcm.wav"):
        recordings.denoise_recordings(nets[0], nets[1], [files[1]["path"], str(bad)], str(out_dir), **SECONDS)
    assert not out_dir.exists() or not os.listdir(out_dir)


def test_mono_false_still_raises(files):
    from sos_amd import audio_io
    with pytest.raises(NotImplementedError):
        audio_io.load_batch_device([files[0]["path"]], mono=False)
    with pytest.raises(NotImplementedError):
        audio_io.load_device(files[0]["path"], mono=False)
