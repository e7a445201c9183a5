"""pipeline.denoise_long(signals=True): the four signals the hand-off writes (the ISTFTs of the mixed, the noise-interval, the
predicted-noise and the output spectrograms) of recordings of any length, cross-faded by ONE sos_window_stitch_planes_f32 launch.
The closed-form networks and the recordings are those of tests/test_gpu_window.py; the reference of the stitch is
tests/window_reference.py (float64): copies bit for bit, blended samples within R.stitch_bound."""
import numpy as np
import pytest
import torch

import sos_amd
import window_reference as R
from oracle import nets as onet

pytestmark = pytest.mark.gpu

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
SECONDS = dict(window_seconds=CORE / 14000, context_seconds=CONTEXT / 14000)
N_ONE, N_LONG = 150 * HOP + 31, 3 * CORE + 5 * HOP + 77
FPS = 25
SIGNALS = ("noisy_input", "noise_intervals", "predicted_full_noise")


@pytest.fixture(scope="module")
def denoiser():
    from sos_amd.common import MyConfig
    from sos_amd.denoiser import networks as jnet
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    return jm.cuda().eval()


@pytest.fixture(scope="module")
def waves():
    """One window's worth and three windows' worth of synthetic noisy speech with frame decisions at 25 frames per second, on
    the GPU.  Never modified."""
    from sos_amd import pipeline
    from sos_amd.dataset import synth_batch

    def wave(seed, n):
        parts = synth_batch(seed, (n + 27999) // 28000)["mixed"]
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(list(parts))[:n])).cuda()

    def bits(seed, n):
        return torch.from_numpy(np.random.default_rng(seed).integers(0, 2, pipeline.n_video_frames(n, 14000, FPS)).astype(np.uint8)).cuda()

    return (wave(700, N_ONE), bits(14, N_ONE)), (wave(710, N_LONG), bits(13, N_LONG))


class _mode:
    def __init__(self, precision):
        self.precision = precision

    def __enter__(self):
        sos_amd.set_precision(self.precision)

    def __exit__(self, *exc):
        sos_amd.set_precision("bf16")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_against_rows(got, wins, rows):
    """`got` (one stitched signal of one recording) against the f64 stitch of its windows' rows."""
    want, blended = R.stitch(wins, rows, CONTEXT)
    bound = R.stitch_bound(wins, rows, CONTEXT)
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    assert _same_bits(got[~blended], want[~blended].astype(np.float32))
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err[blended] <= bound[blended]), float((err[blended] / np.maximum(bound[blended], 1e-300)).max())
    assert blended.sum() == 2 * CONTEXT * (len(wins) - 1)


@pytest.mark.parametrize("precision", ["bf16x3", "fp16"])
def test_a_recording_of_one_window_has_denoise_raggeds_four_signals(denoiser, waves, precision):
    from sos_amd import pipeline
    wave, bits = waves[0]
    assert len(R.plan([N_ONE], CORE, CONTEXT)) == 1
    with _mode(precision):
        outs, extra = pipeline.denoise_long(None, denoiser, [wave], fps=FPS, bits=[bits], signals=True, **SECONDS)
        want, wextra = pipeline.denoise_ragged(None, denoiser, [wave], fps=FPS, bits=[bits], return_all=True)
    assert sorted(extra[0]) == sorted(SIGNALS)
    assert outs[0].shape == (150 * HOP,) and torch.equal(outs[0], want[0])
    for key in SIGNALS:
        assert extra[0][key].shape == (150 * HOP,) and torch.equal(extra[0][key], wextra[0][key]), key
    assert not torch.equal(extra[0]["noisy_input"], outs[0])


@pytest.mark.parametrize("max_batch", [256, 2], ids=["one-group", "two-groups"])
@pytest.mark.parametrize("precision", ["bf16x3", "fp16"])
def test_three_windows_are_the_stitched_rows_of_the_host_cut_windows(denoiser, waves, precision, max_batch):
    from sos_amd import pipeline, tools
    long, bits = waves[1]
    wins = R.plan([N_LONG], CORE, CONTEXT)
    assert len(wins) == 3
    with _mode(precision):
        plain = pipeline.denoise_long(None, denoiser, [long], fps=FPS, bits=[bits], max_batch=max_batch, **SECONDS)
        outs, extra = pipeline.denoise_long(None, denoiser, [long], fps=FPS, bits=[bits], max_batch=max_batch, signals=True,
                                            return_all=True, **SECONDS)
        # the same windows cut on the host, in the groups denoise_long forms of them (longest first)
        _, noise = tools.bits_to_mask_batch(bits[None], 14000 / FPS, N_LONG, long[None])
        groups = pipeline._length_groups([w.samples for w in wins], max_batch, 65536)
        assert len(groups) == (1 if max_batch == 256 else 2)
        rows = [[None] * 3 for _ in range(4)]
        for part in groups:
            ms, B = [wins[i].samples for i in part], len(part)
            wave, masked = torch.zeros((B, max(ms)), device="cuda"), torch.zeros((B, max(ms)), device="cuda")
            for k, i in enumerate(part):
                w = wins[i]
                wave[k, :w.samples], masked[k, :w.samples] = long[w.start:w.start + w.samples], noise[0, w.start:w.start + w.samples]
            rag = pipeline._group_geometry(ms, wave.device, 14000, 30.0, nv=[1] * B)
            y = pipeline._denoise_group_staged(denoiser, wave, masked, rag, signals=True).cpu().numpy()
            assert y.shape[0] == 4 * B
            for q in range(4):
                for k, i in enumerate(part):
                    rows[q][i] = y[q * B + k, :HOP * (wins[i].samples // HOP)]
    assert len(outs) == 1 and outs[0].shape == (3 * CORE + 5 * HOP,)
    assert torch.equal(outs[0], plain[0])                                   # the output is the one without `signals`, bit for bit
    assert set(SIGNALS) | {"plan", "bits", "mask"} == set(extra[0])
    for q, got in enumerate([extra[0][key] for key in SIGNALS] + [outs[0]]):
        _check_against_rows(got, wins, rows[q])
    assert sorted(extra[0]["plan"][:, 7]) == [0, 1, 2]


def test_signals_need_one_decision_stream_per_recording(waves):
    from sos_amd import pipeline
    with pytest.raises(ValueError, match="signals=True"):                   # before any launch: no network is touched
        pipeline.denoise_long(None, None, [waves[0][0]], signals=True, **SECONDS)
    assert pipeline.denoise_long(None, None, [], bits=[], signals=True, **SECONDS) == ([], [])
