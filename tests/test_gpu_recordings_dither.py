"""recordings.denoise_recordings(dither=, dither_seed=): the files written as u8 / s16 / s24 are dithered, the others are written
as before.  bf16x3, the closed-form networks and the files of tests/test_gpu_recordings.py, each about 1 s: stereo s16 at 44.1 kHz,
mono u8 at 8 kHz, an f32 file and a mu-law leg.  The bytes of the dithered encode itself are held against the reference in
tests/test_gpu_dither.py; here: which files it reaches, that a dithered sample is the undithered one within 1 LSB (|d| < 1 moves a
rounding by at most one step), the result rows, and that a call is repeatable."""
import numpy as np
import pytest

import g711_reference as G
import pcm_reference as R
from oracle import nets as onet

pytestmark = pytest.mark.gpu
SECONDS = dict(window_seconds=2.0, context_seconds=0.5)
# name, rate, channels, format, seconds
SPECS = (("pair", 44100, 2, "s16", 1.1), ("byte", 8000, 1, "u8", 1.2), ("float", 14000, 1, "f32", 1.0), ("leg", 8000, 1, "ulaw", 1.2))
PLAIN_KEYS = {"path", "out_path", "channels", "rate", "frames", "format", "clipped", "windows"}


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
    law = fmt in G.TAG
    data, _ = G.encode(planes, fmt) if law else R.encode(planes, fmt)
    path = root / (name + ".wav")
    path.write_bytes(G.container(data, fmt, ch, rate) if law else R.container(data, fmt, ch, rate))
    return dict(name=name, path=str(path), rate=rate, channels=ch, fmt=fmt, frames=n)


@pytest.fixture(scope="module")
def runs(nets, tmp_path_factory):
    """The four files through denoise_recordings without dither, with 'tpdf' twice and with 'highpass': each call once."""
    import sos_amd
    from sos_amd import recordings
    root = tmp_path_factory.mktemp("dither_in")
    files = [_write(root, *spec, seed=67 + i) for i, spec in enumerate(SPECS)]
    paths = [f["path"] for f in files]
    sos_amd.set_precision("bf16x3")
    try:
        out = dict(files=files)
        for name, how in (("plain", {}), ("tpdf", dict(dither="tpdf", dither_seed=3)), ("again", dict(dither="tpdf", dither_seed=3)),
                          ("highpass", dict(dither="highpass", dither_seed=3)), ("seed4", dict(dither="tpdf", dither_seed=4))):
            out[name] = recordings.denoise_recordings(nets[0], nets[1], paths, str(tmp_path_factory.mktemp(name)), **how, **SECONDS)
    finally:
        sos_amd.set_precision("bf16")
    return out


def _bytes(row):
    with open(row["out_path"], "rb") as fp:
        return fp.read()


def _samples(row):
    from sos_amd import audio_io
    return audio_io.read_wave(row["out_path"])[0].astype(np.int64)


def test_files_without_dither_are_byte_equal_to_the_undithered_call(runs):
    for kind in ("tpdf", "highpass"):
        for f, plain, got in zip(runs["files"], runs["plain"], runs[kind]):
            if f["fmt"] in ("f32", "ulaw"):
                assert _bytes(got) == _bytes(plain), (kind, f["name"])
                assert got["dither"] is None and got["clipped"] == plain["clipped"]


def test_dithered_samples_differ_somewhere_and_never_by_more_than_one_lsb(runs):
    for kind in ("tpdf", "highpass"):
        for f, plain, got in zip(runs["files"], runs["plain"], runs[kind]):
            if f["fmt"] in ("s16", "u8"):
                a, b = _samples(plain), _samples(got)
                assert a.shape == b.shape == (f["frames"], f["channels"])
                step = np.abs(a - b)
                print(kind, f["name"], "samples moved:", int((step > 0).sum()), "of", step.size, "largest step", int(step.max()))
                assert step.max() == 1 and got["dither"] == kind
                assert len(_bytes(got)) == len(_bytes(plain))


def test_the_rows_carry_dither_only_when_it_is_asked_for(runs):
    for row in runs["plain"]:
        assert set(row) == PLAIN_KEYS
    for kind in ("tpdf", "highpass"):
        assert [r["dither"] for r in runs[kind]] == [kind, kind, None, None]
        for row, plain in zip(runs[kind], runs["plain"]):
            assert set(row) == PLAIN_KEYS | {"dither"}
            assert {k: row[k] for k in PLAIN_KEYS - {"out_path", "clipped"}} == {k: plain[k] for k in PLAIN_KEYS - {"out_path", "clipped"}}


def test_the_same_call_twice_writes_equal_files_and_another_seed_does_not(runs):
    for f, a, b, c in zip(runs["files"], runs["tpdf"], runs["again"], runs["seed4"]):
        assert _bytes(a) == _bytes(b), f["name"]
        assert a["clipped"] == b["clipped"]
        assert (_bytes(a) != _bytes(c)) == (f["fmt"] in ("s16", "u8")), f["name"]


def test_the_key_is_the_position_in_paths_not_in_the_group(runs, nets, tmp_path, monkeypatch):
    """max_bytes=1 puts every file into a group of its own, where its position is 0: the encode is still handed the position in
    `paths` as the key, one launch per format and group, and the formats without dither are encoded without the arguments."""
    from sos_amd import audio_io, recordings
    calls, encode = [], audio_io.encode_batch_device

    def spy(planes, fmt, **kwargs):
        calls.append((fmt, len(planes), {k: v for k, v in kwargs.items() if k != "frames"}))
        return encode(planes, fmt, **kwargs)

    monkeypatch.setattr(audio_io, "encode_batch_device", spy)
    paths = [f["path"] for f in runs["files"]]
    apart = recordings.denoise_recordings(nets[0], nets[1], paths, str(tmp_path), max_bytes=1, dither="tpdf", dither_seed=3, **SECONDS)
    assert calls == [("s16", 1, dict(dither="tpdf", seed=3, keys=[0])), ("u8", 1, dict(dither="tpdf", seed=3, keys=[1])),
                     ("f32", 1, {}), ("ulaw", 1, {})]
    assert [r["dither"] for r in apart] == ["tpdf", "tpdf", None, None]
    for f, row in zip(runs["files"], apart):
        assert audio_io.wave_info(row["out_path"])["frames"] == f["frames"]
