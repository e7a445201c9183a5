"""recordings.denoise_recordings(loudness=, peak_ceiling_db=) end to end, bf16x3, the closed-form networks of the other recordings
tests.  Four files in one group under high_band='keep': s16 mono at 14 kHz, s16 stereo at 8 kHz, s16 mono at 44.1 kHz (its band
above 7 kHz merged back) and a mu-law leg at 8 kHz.
Bounds.  Bytes: equality with reference_encode(planes_before * g) -- planes_before from the public pieces in the call's order
(tests/test_gpu_band_merge.py's composition), g the float32 gain the call reports, one float32 multiply per sample.  g itself:
2^-22 relative of the reference's (tests/test_gpu_loudness.py).  loudness_before and the 'source' targets: 1e-6 LU of
tests/loudness_reference.py on the same planes.  Reported loudness where the ceiling did not bind: the target within 1e-6 (g is
rounded to float32: 20 log10(1 + 2^-24) = 5e-7 dB).  The s16 file re-read and measured: within 0.05 LU of the reported value --
the s16 step on a signal near -20 LUFS moves the reading by far less, and the margin is for that alone."""
import numpy as np
import pytest
import torch

import g711_reference as G
import loudness_reference as LR
import pcm_reference as R
from oracle import nets as onet

pytestmark = pytest.mark.gpu
SECONDS = dict(window_seconds=2.0, context_seconds=0.5)
SR, TARGET, CEILING = 14000, -20.0, -1.0
# name, rate, channels, format, seconds
SPECS = (("mono", 14000, 1, "s16", 2.5), ("pair", 8000, 2, "s16", 3.0), ("wide", 44100, 1, "s16", 2.5), ("leg", 8000, 1, "ulaw", 3.0))
KEYS = {"loudness_before", "loudness", "loudness_target", "gain_db", "peak_limited"}


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


def _encode(planes, fmt, frames=None):
    return G.encode(planes, fmt, frames) if fmt in G.TAG else R.encode(planes, fmt, frames)


def _container(data, fmt, channels, rate):
    return G.container(data, fmt, channels, rate) if fmt in G.TAG else R.container(data, fmt, channels, rate)


def _stored(f, data=None):
    """What a file holds, as the reference decodes it: (channels, frames) float32."""
    data = f["data"] if data is None else data
    if f["fmt"] in G.TAG:
        return G.decode(np.frombuffer(data, dtype=np.uint8).reshape(-1, f["channels"]), f["fmt"])
    return R.decode(R.unpack(data, f["fmt"], f["channels"]), f["fmt"])


def _write(root, name, rate, ch, fmt, seconds, seed):
    n = int(round(seconds * rate))
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    planes = np.stack([0.3 * np.sin(2 * np.pi * (300 + 70 * c) * t) * (0.2 + (np.sin(2 * np.pi * 1.3 * t + c) > -0.4))
                       + 0.02 * rng.standard_normal(n) for c in range(ch)]).astype(np.float32)
    data, _ = _encode(planes, fmt)
    path = root / (name + ".wav")
    path.write_bytes(_container(data, fmt, ch, rate))
    return dict(name=name, path=str(path), rate=rate, channels=ch, fmt=fmt, frames=n, data=data)


def _compose(nets, files):
    """The public pieces in denoise_recordings' order for one group under high_band='keep': reference decode, to 14 kHz per rate,
    ONE denoise_long, the merge for the rate above 14 kHz and the plain resampling back below it.  -> {name: planes on the host}."""
    from sos_amd import audio_io, windows
    owner = [f for f in files for _ in range(f["channels"])]
    natives = [torch.from_numpy(np.ascontiguousarray(row)).cuda() for f in files for row in _stored(f)]
    clips = list(natives)
    rates = sorted({f["rate"] for f in files} - {SR})
    for rate in rates:
        idx = [k for k, f in enumerate(owner) if f["rate"] == rate]
        for k, y in zip(idx, audio_io.resample_batch_device([natives[k] for k in idx], rate, SR)):
            clips[k] = y
    outs = list(windows.denoise_long(nets[0], nets[1], clips, **SECONDS))
    lows = list(outs)
    for rate in rates:
        idx = [k for k, f in enumerate(owner) if f["rate"] == rate]
        a, b = [clips[k] for k in idx], [lows[k] for k in idx]
        back = audio_io.resample_merge_batch_device([natives[k] for k in idx], a, b, SR, rate, None) if rate > SR \
            else audio_io.resample_batch_device(b, SR, rate)
        for k, y in zip(idx, back):
            outs[k] = y
    planes, k = {}, 0
    for f in files:
        planes[f["name"]] = np.stack([o.cpu().numpy() for o in outs[k:k + f["channels"]]])
        k += f["channels"]
    return planes


def _read(path):
    with open(path, "rb") as fp:
        return fp.read()


@pytest.fixture(scope="module")
def runs(nets, tmp_path_factory):
    """The calls and the composition, computed once and left unchanged; `copies` counts Tensor.cpu on device tensors (the way
    tools/recordings_bench.py counts host waits) during the 'source' call, which runs in several groups."""
    import sos_amd
    from sos_amd import ragged, recordings
    root = tmp_path_factory.mktemp("loud_in")
    files = [_write(root, *spec, seed=91 + i) for i, spec in enumerate(SPECS)]
    paths = [f["path"] for f in files]
    out = lambda name: str(tmp_path_factory.mktemp("loud_" + name))                   # noqa: E731
    sos_amd.set_precision("bf16x3")
    try:
        res = dict(omitted=recordings.denoise_recordings(nets[0], nets[1], paths, out("omitted"), high_band="keep", **SECONDS),
                   none=recordings.denoise_recordings(nets[0], nets[1], paths, out("none"), high_band="keep", loudness=None, **SECONDS),
                   level=recordings.denoise_recordings(nets[0], nets[1], paths, out("level"), high_band="keep", loudness=TARGET,
                                                       peak_ceiling_db=CEILING, **SECONDS))
        planes = _compose(nets, files)
        groups = ragged.byte_groups([4 * f["frames"] * f["channels"] for f in files], 400000)
        copies, orig = [0], torch.Tensor.cpu

        def cpu(self, *a, **k):
            copies[0] += int(self.is_cuda)
            return orig(self, *a, **k)
        torch.Tensor.cpu = cpu
        try:
            res["source"] = recordings.denoise_recordings(nets[0], nets[1], paths, out("source"), loudness="source", max_bytes=400000, **SECONDS)
        finally:
            torch.Tensor.cpu = orig
    finally:
        sos_amd.set_precision("bf16")
    return dict(files=files, res=res, planes=planes, groups=groups, copies=copies[0])


def test_none_writes_the_bytes_of_a_call_without_the_argument(runs):
    for f, a, b in zip(runs["files"], runs["res"]["omitted"], runs["res"]["none"]):
        assert _read(a["out_path"]) == _read(b["out_path"]), f["name"]
        assert set(a) == set(b) == {"path", "out_path", "channels", "rate", "frames", "format", "clipped", "windows"}
        data, clipped = _encode(runs["planes"][f["name"]], f["fmt"], f["frames"])        # and they are the composition's
        assert _read(a["out_path"]) == _container(data, f["fmt"], f["channels"], f["rate"]) and a["clipped"] == clipped


def test_levelled_files_are_the_planes_times_one_gain(runs):
    from sos_amd import audio_io
    for f, r in zip(runs["files"], runs["res"]["level"]):
        assert KEYS <= set(r) and r["loudness_target"] == TARGET, f["name"]
        before = runs["planes"][f["name"]]
        ref = LR.measure(before, f["rate"], None, f["frames"])
        assert np.isfinite(ref["lufs"]) and ref["margin"] > 1e-6, (f["name"], ref)       # the networks' output is not silent
        g = np.float32(10.0 ** (r["gain_db"] / 20.0))
        g_ref, limited = LR.gain(ref["lufs"], ref["peak"], TARGET, CEILING)
        print(f["name"], "before %.6f (reference %.6f), gain %.4f dB, after %.6f, limited %s" % (r["loudness_before"], ref["lufs"], r["gain_db"],
                                                                                           r["loudness"], r["peak_limited"]))
        assert abs(r["loudness_before"] - ref["lufs"]) <= 1e-6 and r["peak_limited"] == limited
        assert abs(float(g) / float(g_ref) - 1.0) <= 2.0 ** -22
        assert r["loudness"] == r["loudness_before"] + r["gain_db"]
        if not r["peak_limited"]:
            assert abs(r["loudness"] - TARGET) <= 1e-6
        else:
            assert r["loudness"] < TARGET
        data, clipped = _encode(LR.apply_gain(before, g, f["frames"]), f["fmt"], f["frames"])
        assert _read(r["out_path"]) == _container(data, f["fmt"], f["channels"], f["rate"]), f["name"]
        assert r["clipped"] == clipped
        tag, bits = (G.TAG[f["fmt"]], 8) if f["fmt"] in G.TAG else R.TAG_BITS[f["fmt"]]
        assert audio_io.wave_info(r["out_path"]) == dict(tag=tag, bits=bits, channels=f["channels"], rate=f["rate"], frames=f["frames"])
        if f["fmt"] == "s16":                                                            # what a meter reads off the written file
            again = LR.measure(_stored(f, data), f["rate"])["lufs"]
            print(f["name"], "re-read: %.6f LUFS" % again)
            assert abs(again - r["loudness"]) <= 0.05


def test_source_targets_are_the_loudness_of_the_decoded_sources(runs):
    for f, r in zip(runs["files"], runs["res"]["source"]):
        ref = LR.measure(_stored(f), f["rate"])
        assert ref["margin"] > 1e-6 and np.isfinite(ref["lufs"])
        print(f["name"], "source %.6f LUFS (reference %.6f), written %.6f" % (r["loudness_target"], ref["lufs"], r["loudness"]))
        assert KEYS <= set(r) and abs(r["loudness_target"] - ref["lufs"]) <= 1e-6
        if not r["peak_limited"]:
            assert abs(r["loudness"] - r["loudness_target"]) <= 1e-6


def test_one_download_per_group(runs):
    assert len(runs["groups"]) == 3 and runs["copies"] == len(runs["groups"])
