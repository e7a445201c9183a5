"""pipeline.StreamDenoiser(high_band='keep' / 'follow'): a live 48 kHz stream comes back with the band above 7 kHz of its input,
bit for bit what resample_merge_batch_device gives the whole signals.  Geometry, networks and precision handling of
tests/test_gpu_stream_resample.py; the 12 kHz statement of tests/test_gpu_band_merge.py."""
import numpy as np
import pytest
import torch

import sos_amd
from oracle import nets as onet

pytestmark = pytest.mark.gpu

SR, RATE, HOP = 14000, 48000, 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
SECONDS = dict(window_seconds=CORE / SR, context_seconds=CONTEXT / SR)
N_LONG = 3 * CORE + 5 * HOP + 77
N_48K = N_LONG * 48 // 14 + 3
N_8K = (CORE + 5 * HOP + 77) * 8 // 14 + 3
TONE, AMP = 12000.0, 0.1
CHUNKS = [5000, 1, 0, 7001, 333]


def _bits(t):
    return t.contiguous().view(torch.int32)


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
def wave48():
    """Synthetic noisy speech taken as a 48 kHz stream, plus a 12 kHz tone of amplitude 0.1, on the GPU.  Never modified."""
    from sos_amd.dataset import synth_batch
    parts = synth_batch(711, (N_48K + 27999) // 28000)["mixed"]
    x = np.concatenate(list(parts))[:N_48K].astype(np.float64)
    x += AMP * np.sin(2 * np.pi * TONE * np.arange(N_48K) / RATE)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _session(sd, x, sizes):
    at, got, i = 0, [], 0
    while at < x.numel():
        n = sizes[i % len(sizes)]
        got.append(sd.push({0: x[at:at + n]})[0])
        at, i = at + n, i + 1
    got.append(sd.close([0])[0])
    return torch.cat(got)


def _run(nets, x, sizes, **kw):
    from sos_amd import pipeline
    sos_amd.set_precision("fp16")
    try:
        sd = pipeline.StreamDenoiser(nets[0], nets[1], 1, max_batch=1, **SECONDS, **kw)
        y = _session(sd, x, sizes)
    finally:
        sos_amd.set_precision("bf16")
    assert sd.plans == [None] and all(rs is None or rs.n_recv == [None] for rs in (sd.rs_in, sd.rs_out))
    assert sd.merger is None or sd.merger.count == [None]
    return y, sd


@pytest.fixture(scope="module")
def runs(nets, wave48):
    """Computed once and left unchanged: a = the stream at 14 kHz, S = a plain StreamDenoiser's output for it, and the sessions
    at 48 kHz without the keyword and under each mode."""
    from sos_amd import audio_io
    a = audio_io.resample_device(wave48, RATE, SR)
    S, _ = _run(nets, a, [4000])
    assert bool(torch.isfinite(S).all()) and S.numel() == a.numel() // HOP * HOP
    out = dict(a=a, S=S, default=_run(nets, wave48, CHUNKS, in_sr=RATE, out_sr=RATE)[0])
    for mode in ("drop", "keep", "follow"):
        out[mode], sd = _run(nets, wave48, CHUNKS, in_sr=RATE, out_sr=RATE, high_band=mode)
        assert (sd.merger is None) == (mode == "drop") and (sd.rs_out is None) == (mode != "drop")
    return out


def test_keep_is_the_file_path_bit_for_bit_with_one_sample_per_input_sample(runs, wave48):
    from sos_amd import audio_io
    want = audio_io.resample_merge_batch_device([wave48], [runs["a"]], [runs["S"]], SR, RATE)[0]
    assert runs["keep"].shape == want.shape == (wave48.numel(),)
    assert torch.equal(_bits(runs["keep"]), _bits(want))


def test_follow_is_the_file_path_with_its_gains_bit_for_bit(runs, wave48):
    from sos_amd import audio_io
    gains = audio_io.band_gains_batch_device([runs["a"]], [runs["S"]], HOP, 2)
    want = audio_io.resample_merge_batch_device([wave48], [runs["a"]], [runs["S"]], SR, RATE, gains)[0]
    assert runs["follow"].shape == want.shape == (wave48.numel(),)
    assert torch.equal(_bits(runs["follow"]), _bits(want))
    assert not torch.equal(_bits(runs["follow"]), _bits(runs["keep"]))


def test_drop_is_the_session_without_the_keyword(runs):
    from sos_amd import audio_io
    assert torch.equal(_bits(runs["drop"]), _bits(runs["default"]))
    assert torch.equal(_bits(runs["drop"]), _bits(audio_io.resample_device(runs["S"], SR, RATE)))


def test_a_rate_below_the_networks_gives_the_same_samples_under_every_mode(nets, wave48):
    x8 = wave48[:N_8K]
    want, _ = _run(nets, x8, CHUNKS, in_sr=8000, out_sr=8000)
    for mode in ("drop", "keep", "follow"):
        got, sd = _run(nets, x8, CHUNKS, in_sr=8000, out_sr=8000, high_band=mode)
        assert sd.merger is None and torch.equal(_bits(got), _bits(want)), mode


def _amplitude(y):
    t = np.arange(len(y)) / RATE
    basis = np.stack([np.sin(2 * np.pi * TONE * t), np.cos(2 * np.pi * TONE * t)], axis=1)
    c, *_ = np.linalg.lstsq(basis, np.asarray(y, dtype=np.float64), rcond=None)
    return float(np.hypot(*c))


def test_keep_returns_the_12_khz_tone_that_drop_loses(runs, wave48):
    n = runs["drop"].numel()
    src, drop, keep = (t.cpu().numpy().astype(np.float64) for t in (wave48[:n], runs["drop"], runs["keep"][:n]))
    a_src, a_drop, a_keep, a_diff = _amplitude(src), _amplitude(drop), _amplitude(keep), _amplitude(keep - drop)
    print("12 kHz amplitude: source %.5f, drop %.3g, keep %.5f, keep - drop %.5f" % (a_src, a_drop, a_keep, a_diff))
    assert abs(a_src - AMP) < 0.02 * AMP
    assert abs(a_diff - a_src) <= 0.02 * a_src
    assert a_drop < 0.01 * a_src                                 # what 'drop' leaves of it


def test_graph_replay_gives_the_eager_bits(nets, runs, wave48):
    got, sd = _run(nets, wave48, CHUNKS, in_sr=RATE, out_sr=RATE, high_band="keep", graph=True)
    assert sd.captures >= 1 and torch.equal(_bits(got), _bits(runs["keep"]))


def test_refusals(nets):
    from sos_amd import pipeline
    for kw, told in ((dict(in_sr=RATE, out_sr=44100, high_band="keep"), "needs in_sr == out_sr"),
                     (dict(in_sr=RATE, high_band="follow"), "needs in_sr == out_sr"),
                     (dict(high_band="keep"), "needs in_sr == out_sr"),
                     (dict(out_sr=RATE, high_band="follow"), "needs in_sr == out_sr"),
                     (dict(in_sr=RATE, out_sr=RATE, high_band="all"), "unknown high_band 'all'"),
                     (dict(in_sr=RATE, out_sr=RATE, high_band="follow", smooth_frames=17), "smooth_frames within 0 .. 16")):
        with pytest.raises(ValueError, match=told):
            pipeline.StreamDenoiser(nets[0], nets[1], 1, **SECONDS, **kw)
