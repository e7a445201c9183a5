"""pipeline.StreamDenoiser: live audio fed in chunks gives denoise_long's result for the same audio.  Geometry, networks and
waves of tests/test_gpu_long_decisions.py (the smallest windows the networks accept)."""
import numpy as np
import pytest
import torch

import sos_amd
import window_reference as R
from conftest import rel_err
from oracle import nets as onet

pytestmark = pytest.mark.gpu

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
SECONDS = dict(window_seconds=CORE / 14000, context_seconds=CONTEXT / 14000)
N_ONE, N_LONG, N_TWO, N_OTHER, N_STEPS = 150 * HOP + 31, 3 * CORE + 5 * HOP + 77, 2 * CORE + 3 * HOP + 5, 14000 + 157, 5 * CORE + 100
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
    """Three windows, two windows, one window, another single window, and two of five cores: synthetic noisy speech on the GPU.
    Never modified."""
    from sos_amd.dataset import synth_batch

    def wave(seed, n):
        parts = synth_batch(seed, (n + 27999) // 28000)["mixed"]
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(list(parts))[:n])).cuda()

    return dict(long=wave(710, N_LONG), two=wave(730, N_TWO), one=wave(700, N_ONE), other=wave(720, N_OTHER),
                left=wave(740, N_STEPS), right=wave(750, N_STEPS))


class _mode:
    def __init__(self, precision):
        self.precision = precision

    def __enter__(self):
        sos_amd.set_precision(self.precision)

    def __exit__(self, *exc):
        sos_amd.set_precision("bf16")


FOUR = ("long", "two", "one", "other")


@pytest.fixture(scope="module")
def offline(nets, waves):
    """denoise_long of the four recordings, every window alone (max_batch = 1) and in shared batches (the default), per
    precision.  Existing code alone; never modified."""
    from sos_amd import pipeline
    det, jm = nets
    res = {}
    for precision in PRECISIONS:
        with _mode(precision):
            alone = pipeline.denoise_long(det, jm, [waves[k] for k in FOUR], max_batch=1, **SECONDS)
            shared = pipeline.denoise_long(det, jm, [waves[k] for k in FOUR], **SECONDS)
        res[precision] = dict(alone=dict(zip(FOUR, alone)), shared=dict(zip(FOUR, shared)))
    return res


# {slot: [(stream, chunk size), ...]}: `one` ends first, is closed at once and its slot used again for `other`.
#   cadences: the streams advance at different rates, so no two windows are ever ready in the same call
#   lock step: `long` and `two` run their first windows in one step, `two` and `one`, then `long` and `other` are closed together
SCENARIOS = {"cadences": {0: [("long", 1000)], 1: [("two", 4099)], 2: [("one", 700), ("other", 5000)]},
             "lock step": {0: [("long", 5000)], 1: [("two", 5000)], 2: [("one", N_ONE), ("other", N_OTHER)]}}


def _three_slots(sd, waves, scenario):
    """The four streams through three slots; slot 1 gets host chunks.  -> (the streams' outputs, the most windows in one step)."""
    plan = {s: list(todo) for s, todo in SCENARIOS[scenario].items()}
    most, run = [0], sd._run
    sd._run = lambda items, *a: (most.__setitem__(0, max(most[0], len(items))), run(items, *a))[1]
    at, outs = {s: 0 for s in plan}, {k: [] for k in FOUR}
    while plan:
        chunks = {}
        for s, todo in plan.items():
            name, size = todo[0]
            c = waves[name][at[s]:at[s] + size]
            chunks[s] = c.cpu().numpy() if s == 1 else c
            at[s] += c.numel()
        for s, y in sd.push(chunks).items():
            outs[plan[s][0][0]].append(y)
        ended = [s for s, todo in plan.items() if at[s] >= waves[todo[0][0]].numel()]
        if scenario == "lock step" and ended == [2] and len(plan) > 1:
            continue                                            # slot 2 waits (with empty chunks) until another stream ends too
        if ended:
            for s, y in sd.close(ended).items():
                outs[plan[s].pop(0)[0]].append(y)
                at[s] = 0
                if not plan[s]:
                    del plan[s]
    return {k: torch.cat(v) for k, v in outs.items()}, most[0]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_stream_in_chunks_is_denoise_long_bit_for_bit(nets, waves, offline, precision):
    from sos_amd import pipeline
    det, jm = nets
    x = waves["long"]
    assert len(R.plan([N_LONG], CORE, CONTEXT)) == 3 and N_LONG % 1000 % 2 == 1
    with _mode(precision):
        sd = pipeline.StreamDenoiser(det, jm, 1, **SECONDS)
        got = [sd.push({0: x[i:i + 1000]})[0] for i in range(0, N_LONG, 1000)]
        got.append(sd.close([0])[0])
    lens = [int(g.numel()) for g in got]
    # window k runs with the chunk that brings sample (k + 2) core; what it makes final ends at (k + 1) core - context
    assert [n for n in lens if n] == [CORE - CONTEXT, CORE, N_LONG // HOP * HOP - 2 * CORE + CONTEXT]
    assert lens.index(CORE - CONTEXT) == (2 * CORE - 1) // 1000 and lens.index(CORE) == (3 * CORE - 1) // 1000
    want = offline[precision]["alone"]["long"]
    assert bool(torch.isfinite(want).all()) and torch.equal(torch.cat(got), want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_short_stream_is_denoise_raggeds_clip(nets, waves, precision):
    from sos_amd import pipeline
    det, jm = nets
    with _mode(precision):
        want = pipeline.denoise_ragged(det, jm, [waves["one"]])[0]
        sd = pipeline.StreamDenoiser(det, jm, 2, **SECONDS)
        assert sd.push({1: waves["one"][:9999]})[1].numel() == 0 and sd.push({1: waves["one"][9999:]})[1].numel() == 0
        got = sd.close(1)[1]
    assert got.shape == (150 * HOP,) and torch.equal(got, want)


@pytest.mark.parametrize("scenario", list(SCENARIOS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_three_slots_one_of_them_used_twice_are_denoise_long_bit_for_bit(nets, waves, offline, precision, scenario):
    from sos_amd import pipeline
    det, jm = nets
    with _mode(precision):
        got, most = _three_slots(pipeline.StreamDenoiser(det, jm, 3, max_batch=1, **SECONDS), waves, scenario)
    assert most == (2 if scenario == "lock step" else 1)
    for k in FOUR:
        assert torch.equal(got[k], offline[precision]["alone"][k]), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_shared_batches_stay_within_twice_what_sharing_costs_denoise_long(nets, waves, offline, precision):
    """The margin is measured on existing code: the largest relative distance between denoise_long with every window alone and
    with its default batches, on the same recordings; a stream's batches are a third composition, hence twice that."""
    from sos_amd import pipeline
    det, jm = nets
    alone, shared = offline[precision]["alone"], offline[precision]["shared"]
    cost = max(rel_err(shared[k].cpu().numpy(), alone[k].cpu().numpy()) for k in FOUR)
    with _mode(precision):
        got, most = _three_slots(pipeline.StreamDenoiser(det, jm, 3, **SECONDS), waves, "lock step")
    assert most == 2                                            # windows of two streams shared their groups
    dist = {k: rel_err(got[k].cpu().numpy(), alone[k].cpu().numpy()) for k in FOUR}
    print(precision, "denoise_long shared against alone %.3e; streams against alone" % cost, {k: "%.3e" % v for k, v in dist.items()})
    for k in FOUR:
        assert got[k].shape == alone[k].shape and bool(torch.isfinite(got[k]).all())
        assert torch.equal(got[k], alone[k]) if cost == 0 else dist[k] <= 2 * cost, (k, dist[k], cost)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_graphed_steps_are_the_eager_steps_and_each_shape_is_captured_once(nets, waves, precision):
    from sos_amd import pipeline
    det, jm = nets
    sizes = [2 * CORE, CORE, CORE, CORE]                        # two slots in lock step: one window each per call
    with _mode(precision):
        res = []
        for graph in (False, True):
            sd = pipeline.StreamDenoiser(det, jm, 2, graph=graph, **SECONDS)
            at, outs = 0, []
            for n in sizes:
                outs.append(sd.push({0: waves["left"][at:at + n], 1: waves["right"][at:at + n]}))
                at += n
            sd.drop([0, 1])
            res.append((outs, sd.captures))
    (eager, none), (graphed, captures) = res
    assert none == 0 and captures == 2                          # (core + context) x 2 and (core + 2 context) x 2
    for a, b, n in zip(eager, graphed, [CORE - CONTEXT, CORE, CORE, CORE]):
        for s in (0, 1):
            assert a[s].shape == (n,) and torch.equal(a[s], b[s]) and bool(torch.isfinite(b[s]).all())
    assert not torch.equal(eager[1][0], eager[1][1])


def test_nothing_synchronises_during_push_after_a_warm_up_session(nets, waves):
    from sos_amd import pipeline
    det, jm = nets
    x, host = waves["two"], waves["two"].cpu().numpy()
    with _mode("fp16"):
        outs = []
        for debug in ("default", "error"):
            sd = pipeline.StreamDenoiser(det, jm, 2, **SECONDS)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode(debug)
            try:
                got = [sd.push({0: x[i:i + 5000], 1: host[i:i + 5000]}) for i in range(0, N_TWO, 5000)]
            finally:
                torch.cuda.set_sync_debug_mode("default")
            outs.append(torch.cat([g[s] for g in got for s in (0, 1)] + list(sd.close([0, 1]).values())))
    assert outs[0].numel() == 2 * (N_TWO // HOP * HOP) and torch.equal(outs[0], outs[1])


def test_refusals_come_before_any_launch(nets, waves):
    from sos_amd import pipeline
    det, jm = nets
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(ValueError, match="twice the context"):
            pipeline.StreamDenoiser(None, None, 1, window_seconds=CORE / 14000, context_seconds=(CORE // 2 + HOP) / 14000)
        with pytest.raises(ValueError, match="65 hops"):
            pipeline.StreamDenoiser(None, None, 1, window_seconds=40 * HOP / 14000, context_seconds=CONTEXT / 14000)
        with pytest.raises(ValueError, match="slots"):
            pipeline.StreamDenoiser(None, None, 0, **SECONDS)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sd = pipeline.StreamDenoiser(None, None, 2, **SECONDS)       # no network is touched below
    for slot in (2, -1, "0"):
        with pytest.raises(ValueError, match="unknown slot"):
            sd.push({slot: waves["one"]})
    for chunk in (waves["one"][None], waves["one"].double(), waves["one"].cpu().numpy().astype(np.float64), [0.0] * 10):
        with pytest.raises(ValueError, match="1-D float32"):
            sd.push({0: chunk})
    assert sd.plans == [None, None]                             # nothing was opened
    for call in (sd.close, sd.drop):
        with pytest.raises(ValueError, match="slot 1 has no open stream"):
            call([1])
    sd.push({0: waves["one"][:64 * HOP - 1], 1: waves["one"][:100]})
    with pytest.raises(ValueError, match="slot 0 got 10111 samples; slot 1 got 100 samples"):
        sd.close([0, 1])
    with pytest.raises(ValueError, match="slot 0 has no open stream"):
        sd.close([0])
    with _mode("fp16"):                                         # the slot can be used again
        sd = pipeline.StreamDenoiser(det, jm, 2, **SECONDS)
        sd.push({0: waves["one"][:50]})
        with pytest.raises(ValueError, match="slot 0 got 50 samples"):
            sd.close(0)
        sd.push({0: waves["one"]})
        assert sd.close(0)[0].shape == (150 * HOP,)
