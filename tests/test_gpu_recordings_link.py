"""recordings.denoise_recordings(link_channels=): the channels of a file silenced by ONE shared stream of decisions.  One stereo
16-bit file at 44.1 kHz (two windows per channel) and one mono float file at 14 kHz (one window), bf16x3, the closed-form
networks of tests/test_gpu_recordings.py.  The bound is equality: the written bytes are those of the same chain done by public
pieces -- load_channels_batch_device, ONE denoise_long over all channels, resample back, encode_batch_device, wave_container."""
import os

import numpy as np
import pytest

from oracle import nets as onet

pytestmark = pytest.mark.gpu
SECONDS = dict(window_seconds=1.0, context_seconds=0.25)
KEYS = {"path", "out_path", "channels", "rate", "frames", "format", "clipped", "windows"}
# name, rate, channels, format, seconds
SPECS = (("stereo", 44100, 2, "s16", 2.2), ("mono", 14000, 1, "f32", 1.5))
WINDOWS = dict(stereo=4, mono=1)


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


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The two sources, written with audio_io.wave_container."""
    from sos_amd import audio_io
    root = tmp_path_factory.mktemp("link_in")
    out = []
    for i, (name, rate, ch, fmt, seconds) in enumerate(SPECS):
        n = int(round(seconds * rate))
        rng = np.random.default_rng(71 + i)
        t = np.arange(n) / rate
        # channels the detector decides differently: amplitude-modulated noise and a chirp
        chans = [0.3 * rng.standard_normal(n) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.8 * t)) ** 4,
                 0.4 * np.sin(2 * np.pi * (100 + 3000 * t / t[-1]) * t)]
        sig = np.stack(chans[:ch], axis=1).astype(np.float32)
        data = np.clip(np.rint(sig * 32768.0), -32768, 32767).astype(np.int16) if fmt == "s16" else sig
        tag, bits = audio_io.ENCODINGS[fmt][2:]
        path = root / (name + ".wav")
        path.write_bytes(audio_io.wave_container(data.tobytes(), tag, ch, rate, bits))
        out.append(dict(name=name, path=str(path), rate=rate, channels=ch, fmt=fmt, frames=n, tag=tag, bits=bits))
    return out


def _by_pieces(nets, files, **how):
    """The chain of denoise_recordings out of public pieces, denoise_long run as `how` says (link='owner': the file of each
    channel): -> the files' bytes by name."""
    from sos_amd import audio_io, pipeline, windows
    ys, _, _ = audio_io.load_channels_batch_device([f["path"] for f in files], sr=pipeline.SR)
    owner = [k for k, y in enumerate(ys) for _ in range(y.shape[0])]
    clips = [y[c] for y in ys for c in range(y.shape[0])]
    if how.get("link") == "owner":
        how = dict(how, link=owner)
    outs = list(windows.denoise_long(nets[0], nets[1], clips, **SECONDS, **how))
    for rate in sorted({f["rate"] for f in files} - {pipeline.SR}):
        idx = [k for k, o in enumerate(owner) if files[o]["rate"] == rate]
        for k, y in zip(idx, audio_io.resample_batch_device([outs[k] for k in idx], pipeline.SR, rate)):
            outs[k] = y
    blobs, k = {}, 0
    for f in files:
        planes = audio_io.planes_of(outs[k:k + f["channels"]])
        k += f["channels"]
        data, offsets, _ = audio_io.encode_batch_device([planes], f["fmt"], frames=[f["frames"]])
        assert int(offsets[1]) == f["frames"] * f["channels"] * f["bits"] // 8
        blobs[f["name"]] = audio_io.wave_container(data.cpu().numpy().tobytes(), f["tag"], f["channels"], f["rate"], f["bits"])
    return blobs


def _run(nets, files, out_dir, **kw):
    from sos_amd import recordings
    res = recordings.denoise_recordings(nets[0], nets[1], [f["path"] for f in files], str(out_dir), **SECONDS, **kw)
    return res, {f["name"]: open(r["out_path"], "rb").read() for f, r in zip(files, res)}


@pytest.fixture(scope="module")
def linked(nets, files, tmp_path_factory):
    """denoise_recordings(link_channels='any') and the chains it is compared with: computed once and left unchanged."""
    import sos_amd
    sos_amd.set_precision("bf16x3")
    try:
        res, written = _run(nets, files, tmp_path_factory.mktemp("link_out"), link_channels="any")
        pieces = _by_pieces(nets, files, stitch_bits=True, link="owner")
        unlinked = _by_pieces(nets, files, stitch_bits=True)
    finally:
        sos_amd.set_precision("bf16")
    return res, written, pieces, unlinked


def test_outputs_keep_frames_channels_rate_and_format_and_the_eight_keys(linked, files):
    from sos_amd import audio_io
    res, _, _, _ = linked
    assert [r["path"] for r in res] == [f["path"] for f in files]
    for f, r in zip(files, res):
        assert audio_io.wave_info(r["out_path"]) == dict(tag=f["tag"], bits=f["bits"], channels=f["channels"], rate=f["rate"], frames=f["frames"])
        assert (r["channels"], r["rate"], r["frames"], r["format"]) == (f["channels"], f["rate"], f["frames"], f["fmt"])
        assert set(r) == KEYS and r["windows"] == WINDOWS[f["name"]]


def test_written_bytes_are_the_chain_by_pieces_with_the_files_as_link_groups(linked, files):
    _, written, pieces, unlinked = linked
    for f in files:
        assert written[f["name"]] == pieces[f["name"]], f["name"]
    # a mono file is a group of one: what stitch_bits gives it without any link
    assert written["mono"] == unlinked["mono"]
    # the condition without which the above shows nothing: the channels' own streams differ, so sharing one changes the file
    differ = sum(a != b for a, b in zip(written["stereo"], unlinked["stereo"]))
    print("stereo bytes that differ from per-channel streams:", differ, "of", len(written["stereo"]))
    assert len(written["stereo"]) == len(unlinked["stereo"]) and differ > 0


def test_mean_runs_the_same_chain(nets, files, tmp_path):
    res, written = _run(nets, files, tmp_path, link_channels="mean")
    pieces = _by_pieces(nets, files, stitch_bits=True, link="owner", link_mode="mean")
    assert all(set(r) == KEYS for r in res) and written == pieces


def test_link_channels_none_is_the_default_chain(nets, files, tmp_path):
    res, written = _run(nets, files, tmp_path / "none", link_channels=None)
    _, default = _run(nets, files, tmp_path / "default")
    pieces = _by_pieces(nets, files)
    assert all(set(r) == KEYS for r in res) and written == pieces and default == pieces


def test_an_unknown_value_is_refused_and_nothing_is_written(nets, files, tmp_path):
    from sos_amd import recordings
    out_dir = tmp_path / "out"
    with pytest.raises(ValueError, match="link_channels"):
        recordings.denoise_recordings(nets[0], nets[1], [f["path"] for f in files], str(out_dir), link_channels="max", **SECONDS)
    assert not out_dir.exists() or not os.listdir(out_dir)
