"""pipeline.detect_long and denoise_long(stitch_bits=True): one stream of frame decisions per recording of any length, and the
recording silenced by that one stream.  Geometry, networks and waves of tests/test_gpu_window.py (the smallest windows the
networks accept); the float64 stitch of the per-window logits is tests/frames_reference.py."""
import numpy as np
import pytest
import torch

import frames_reference as FR
import sos_amd
import window_reference as R
from oracle import nets as onet

pytestmark = pytest.mark.gpu

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
SECONDS = dict(window_seconds=CORE / 14000, context_seconds=CONTEXT / 14000)
N_ONE, N_LONG = 150 * HOP + 31, 3 * CORE + 5 * HOP + 77
PRECISIONS = ["bf16x3", "fp16"]


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
def waves():
    """One window's worth, three windows' worth, and another short one: synthetic noisy speech, on the GPU.  Never modified."""
    from sos_amd.dataset import synth_batch

    def wave(seed, n):
        parts = synth_batch(seed, (n + 27999) // 28000)["mixed"]
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(list(parts))[:n])).cuda()

    return wave(700, N_ONE), wave(710, N_LONG), wave(720, 14000 + 157)


class _mode:
    def __init__(self, precision):
        self.precision = precision

    def __enter__(self):
        sos_amd.set_precision(self.precision)

    def __exit__(self, *exc):
        sos_amd.set_precision("bf16")


@pytest.fixture(scope="module")
def long_runs(nets, waves):
    """The three-window recording, once per precision and left unchanged: detect_long, and denoise_long's default path with its
    per-window logits."""
    from sos_amd import pipeline
    det, jm = nets
    res = {}
    for precision in PRECISIONS:
        with _mode(precision):
            pairs, dextra = pipeline.detect_long(det, [waves[1]], return_all=True, **SECONDS)
            out, extra = pipeline.denoise_long(det, jm, [waves[1]], return_all=True, **SECONDS)
        res[precision] = dict(pairs=pairs, dextra=dextra, out=out, extra=extra)
    return res


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_recording_of_one_window_is_denoise_ragged(nets, waves, precision):
    from sos_amd import pipeline
    det, jm = nets
    assert len(R.plan([N_ONE], CORE, CONTEXT)) == 1
    with _mode(precision):
        want, wextra = pipeline.denoise_ragged(det, jm, [waves[0]], return_all=True)
        pairs = pipeline.detect_long(det, [waves[0]], **SECONDS)
        got, extra = pipeline.denoise_long(det, jm, [waves[0]], stitch_bits=True, return_all=True, **SECONDS)
    logits, bits = pairs[0]
    assert logits.shape == bits.shape == (pipeline.n_video_frames(N_ONE),) and bits.dtype == torch.uint8
    assert torch.equal(logits, wextra[0]["logits"]) and torch.equal(bits, wextra[0]["bits"])
    assert got[0].shape == (150 * HOP,) and torch.equal(got[0], want[0])
    assert torch.equal(extra[0]["logits"], logits) and torch.equal(extra[0]["bits"], bits) and extra[0]["mask"].shape == (N_ONE,)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_three_windows_are_the_float64_stitch_of_the_windows_logits(long_runs, precision):
    from sos_amd import pipeline, tools
    run = long_runs[precision]
    (logits, bits), windows = run["pairs"][0], run["extra"][0]["windows"]
    wins = R.plan([N_LONG], CORE, CONTEXT)
    F = pipeline.n_video_frames(N_LONG)
    assert len(wins) == 3 and logits.shape == bits.shape == (F,)
    rows = [w["logits"].cpu().numpy() for w in windows]
    assert [len(r) for r in rows] == FR.window_frames(wins, 14000, 30.0)
    # detect_long ran the same windows in the same groups as denoise_long's default path: the same per-window logits
    assert all(torch.equal(a, b["logits"]) for a, b in zip(run["dextra"][0]["windows"], windows))
    st = FR.stitch(wins, rows, 14000, 30.0, CORE, CONTEXT)
    got = logits.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got[~st.blended].view(np.uint32), st.out[~st.blended].astype(np.float32).view(np.uint32))
    err = np.abs(got.astype(np.float64) - st.out)
    print(precision, "frames", F, "blended", int(st.blended.sum()), "max err / bound %.3f" % float((err[st.blended] / np.maximum(st.bound[st.blended], 1e-300)).max()))
    assert 5 <= st.blended.sum() <= 23 and np.all(err <= st.bound)
    # the bits are the threshold applied to the returned logits
    assert torch.equal(bits, tools.threshold_bits(logits, pipeline.SIGMOID_THRESHOLD)[0])
    # denoise_long(return_all=True) carries the same stitched stream next to its windows
    assert torch.equal(run["extra"][0]["logits"], logits) and torch.equal(run["extra"][0]["bits"], bits)


@pytest.mark.parametrize("max_batch", [256, 2], ids=["one-group", "two-groups"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stitch_bits_is_the_bits_path_on_detect_longs_bits(nets, waves, precision, max_batch):
    from sos_amd import pipeline
    det, jm = nets
    with _mode(precision):
        pairs = pipeline.detect_long(det, [waves[1]], max_batch=max_batch, **SECONDS)
        got, extra = pipeline.denoise_long(det, jm, [waves[1]], stitch_bits=True, max_batch=max_batch, return_all=True, **SECONDS)
        want, wextra = pipeline.denoise_long(None, jm, [waves[1]], bits=[pairs[0][1]], fps=30.0, max_batch=max_batch, return_all=True, **SECONDS)
    assert got[0].shape == (3 * CORE + 5 * HOP,) and torch.equal(got[0], want[0]) and bool(torch.isfinite(got[0]).all())
    assert torch.equal(extra[0]["bits"], pairs[0][1]) and torch.equal(extra[0]["logits"], pairs[0][0])
    assert torch.equal(extra[0]["mask"], wextra[0]["mask"]) and np.array_equal(extra[0]["plan"], wextra[0]["plan"])
    assert sorted(extra[0]) == ["bits", "logits", "mask", "plan"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_bits_path_stages_slices_of_the_full_length_noise_intervals(nets, waves, precision):
    """Guards the rewrite of the `bits=` path onto sos_window_stage_masked_f32: the same output as staging the windows on the
    host out of tools.ragged_stage's full-length rows, at 25 frames per second, two recordings of different lengths."""
    from sos_amd import pipeline, ragged, tools
    _, jm = nets
    clips, rates = [waves[1], waves[0]], [25.0, 30.0]
    ns = [N_LONG, N_ONE]
    rng = np.random.default_rng(13)
    bits = [torch.from_numpy(rng.integers(0, 2, pipeline.n_video_frames(n, 14000, f)).astype(np.uint8)).cuda() for n, f in zip(ns, rates)]
    wins = R.plan(ns, CORE, CONTEXT)
    with _mode(precision):
        got, extra = pipeline.denoise_long(None, jm, clips, fps=rates, bits=bits, return_all=True, **SECONDS)
        full_wave, full_masked, full_mask = tools.ragged_stage(torch.cat(clips), ragged.clip_table(ns, [len(b) for b in bits]), max(ns),
                                                              torch.cat(bits), [14000 / f for f in rates])
        order = pipeline._length_groups([w.samples for w in wins], 256, 65536)
        assert len(order) == 1
        ms = [wins[i].samples for i in order[0]]
        wave, masked = torch.zeros((4, max(ms)), device="cuda"), torch.zeros((4, max(ms)), device="cuda")
        for k, i in enumerate(order[0]):
            w = wins[i]
            wave[k, :w.samples] = full_wave[w.recording, w.start:w.start + w.samples]
            masked[k, :w.samples] = full_masked[w.recording, w.start:w.start + w.samples]
        nv = [max(1, pipeline.n_video_frames(wins[i].samples, 14000, rates[wins[i].recording])) for i in order[0]]
        y = pipeline._denoise_group_staged(jm, wave, masked, pipeline._group_geometry(ms, wave.device, 14000, 30.0, nv=nv))
        rows = torch.zeros_like(y)
        for k, i in enumerate(order[0]):
            rows[i] = y[k]
        tab = R.table(wins, ns)
        tab[:, 2] = HOP * (tab[:, 2] // HOP)
        want = tools.window_stitch(rows, tab, CONTEXT)
    assert torch.equal(torch.cat(got), want) and bool(torch.isfinite(want).all())
    for e, m, b in zip(extra, ragged.split(full_mask, ns), bits):
        assert torch.equal(e["mask"], m) and torch.equal(e["bits"], b)
    assert 0 < float(full_mask.sum()) < sum(ns)


def test_stitch_bits_with_bits_raises_before_any_launch(nets, waves):
    from sos_amd import pipeline
    det, jm = nets
    bits = [torch.zeros(pipeline.n_video_frames(N_ONE), dtype=torch.uint8, device="cuda")]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(ValueError, match="stitch_bits"):
            pipeline.denoise_long(None, None, [waves[0]], bits=bits, stitch_bits=True, **SECONDS)      # no network is touched
    finally:
        torch.cuda.set_sync_debug_mode("default")
    with pytest.raises(ValueError, match="recording 1"):
        pipeline.detect_long(det, [waves[0], torch.zeros(64 * HOP - 1, device="cuda")], **SECONDS)
    with pytest.raises(ValueError):
        pipeline.detect_long(det, [waves[0]], n_frames=[3, 4], **SECONDS)
    assert pipeline.detect_long(det, [], **SECONDS) == []


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_mixed_list_returns_in_input_order_and_nothing_synchronises(nets, waves, precision):
    """[short, long, short]: with one window per group (max_batch = 1) every window runs exactly as in a list of its own, so
    each entry equals its stand-alone result bit for bit.  The second calls run under torch.cuda.set_sync_debug_mode('error'):
    nothing waits for the device between the groups (the first calls built plans, tables and workspaces)."""
    from sos_amd import pipeline
    det, jm = nets
    clips = [waves[0], waves[1], waves[2]]
    with _mode(precision):
        alone = [pipeline.detect_long(det, [c], max_batch=1, **SECONDS)[0] for c in clips]
        pipeline.detect_long(det, clips, max_batch=1, **SECONDS)
        pipeline.denoise_long(det, jm, clips, stitch_bits=True, max_batch=2, **SECONDS)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = pipeline.detect_long(det, clips, max_batch=1, **SECONDS)
            grouped = pipeline.detect_long(det, clips, **SECONDS)
            outs = pipeline.denoise_long(det, jm, clips, stitch_bits=True, max_batch=2, **SECONDS)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    for (lg, b), (alg, ab), (glg, gb), c in zip(got, alone, grouped, clips):
        F = pipeline.n_video_frames(c.numel())
        assert lg.shape == b.shape == glg.shape == gb.shape == (F,)
        assert torch.equal(lg, alg) and torch.equal(b, ab) and bool(torch.isfinite(glg).all())
    for o, c in zip(outs, clips):
        assert o.shape == (HOP * (c.numel() // HOP),) and bool(torch.isfinite(o).all())


def test_one_rate_and_one_frame_count_per_recording(nets, waves):
    """fps per recording and n_frames: the hand-off's labels are not always n_video_frames long.  A one-window recording with
    F frames is that clip with F video frames (max_batch = 1: alone in its group, so bit for bit); a three-window recording
    gets F stitched frames."""
    from sos_amd import pipeline, transform
    det, _ = nets
    F_one, F_long = pipeline.n_video_frames(N_ONE, 14000, 25.0) - 1, pipeline.n_video_frames(N_LONG, 14000, 29.97) + 2
    with _mode("bf16x3"):
        pairs = pipeline.detect_long(det, [waves[0], waves[1]], fps=[25.0, 29.97], n_frames=[F_one, F_long], max_batch=1, **SECONDS)
        rag = pipeline._group_geometry([N_ONE], waves[0].device, 14000, 25.0, nv=[F_one])
        want = pipeline.detect(det, transform.stft_batch(waves[0][None].contiguous(), clip_samples=rag.tab(rag.n_samples)), F_one, rag=rag)
    assert pairs[0][0].shape == (F_one,) and pairs[1][0].shape == pairs[1][1].shape == (F_long,)
    assert bool(torch.isfinite(pairs[1][0]).all()) and torch.equal(pairs[0][0], want[0])
