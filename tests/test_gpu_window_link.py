"""sos_window_frames_link_f32 (csrc/ragged_window.hip) and detect_long / denoise_long(link=): ONE decision stream shared by the
recordings of a group.  Kernel level first -- random logit rows, no networks: the group logits are tests/link_reference.py's
reduction of what tools.window_frames_stitch gives each member on the same rows, bit for bit, and the bits are
tools.threshold_bits of them, bit for bit -- then end to end with the networks and waves of tests/test_gpu_long_decisions.py."""
import numpy as np
import pytest
import torch

import frames_reference as FR
import link_reference as LR
import sos_amd
import window_reference as R
from oracle import nets as onet

gpu = pytest.mark.gpu

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
SR, FPS = 14000, 30.0
SECONDS = dict(window_seconds=CORE / SR, context_seconds=CONTEXT / SR)
N_ONE, N_LONG = 150 * HOP + 31, 3 * CORE + 5 * HOP + 77
# a trio of one-window recordings, a pair of three-window recordings, a single one-window recording and an unlinked one of
# twelve windows between them; no two members of a group are neighbours
NS = [N_ONE, N_LONG, 100 * HOP + 5, N_ONE, 12 * CORE + 3 * HOP, N_LONG, N_ONE]
IDS = ["trio", "pair", None, "trio", None, "pair", "trio"]
SEED = 17
PRECISIONS = ["bf16x3", "fp16"]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _case():
    """Plan, table (rows permuted: a recording's windows sit in unrelated rows), frame counts, random rows with the special
    logits, the recordings' table and the link tables.  Host only."""
    wins = R.plan(NS, CORE, CONTEXT)
    tab = R.table(wins, NS)
    wf, recs, foff = [], [], 0
    for r, n in enumerate(NS):
        mine = [w for w in wins if w.recording == r]
        F = FR.n_video_frames(n, SR, FPS)
        recs.append((foff, F, len(wf), len(mine)))
        wf += FR.window_frames(mine, SR, FPS)
        foff += F
    recs = np.asarray(recs, dtype=np.int64)
    rng = np.random.default_rng(SEED)
    rows = rng.standard_normal((len(wins), max(wf) + 3)).astype(np.float32)
    first = recs[:, 2]
    rows[first[2], 0] = 0.0                                     # a group of one: exactly the threshold
    rows[first[4], 1], rows[first[4], 2] = 1e-7, -1e-7          # the unlinked recording: next to it
    rows[first[1], 5], rows[first[5], 5] = 0.25, -0.25          # the pair: its mean is exactly 0 in a frame that is copied
    order = rng.permutation(len(wins))
    moved = np.zeros_like(rows)
    moved[order] = rows
    tab[:, 7] = order
    links, members, group = LR.tables(IDS, recs[:, 1])
    return dict(wins=wins, tab=tab, wf=np.asarray(wf, dtype=np.int64), recs=recs, rows=moved, plain_rows=rows, links=links,
                members=members, group=group)


def test_the_seed_leaves_the_reference_decision_to_rounding_in_at_most_one_percent_of_the_frames():
    """No GPU: the float64 stitch of the same rows, reduced and decided by the reference alone."""
    c = _case()
    assert [int(k) for k in c["recs"][:, 3]] == [1, 3, 1, 1, 12, 3, 1] and c["links"][:, 3].tolist() == [3, 2, 1, 1]
    assert sorted(c["tab"][:, 7].tolist()) == list(range(len(c["tab"]))) and not np.array_equal(c["tab"][:, 7], np.arange(len(c["tab"])))
    for context in (CONTEXT, 0):
        per_rec = []
        for r, (_, F, first, K) in enumerate(c["recs"]):
            mine = [w for w in c["wins"] if w.recording == r]
            st = FR.stitch(mine, [c["plain_rows"][first + k, :c["wf"][first + k]] for k in range(K)], SR, FPS, CORE, context)
            per_rec.append(st.out.astype(np.float32))
        for mode in LR.MODES:
            streams = [LR.link([per_rec[m] for m in c["members"][f:f + n]], mode) for _, _, f, n in c["links"]]
            x = np.concatenate(streams)
            near = LR.near_threshold(x)
            print(mode, "context", context, "frames", len(x), "near the threshold", int(near.sum()))
            assert len(x) == int(c["links"][:, 1].sum()) >= 400 and 3 <= near.sum() <= 0.01 * len(x)
            assert (x == 0.0).sum() >= (2 if mode == "mean" else 1)


@gpu
@pytest.mark.parametrize("context", [CONTEXT, 0])
def test_group_streams_are_the_reference_reduction_of_the_members_stitched_streams(context):
    from sos_amd import tools
    c = _case()
    d_rows = torch.from_numpy(c["rows"]).cuda()
    ratio = SR / FPS
    flat = tools.window_frames_stitch(d_rows, c["tab"], c["wf"], c["recs"], ratio, CORE, context)
    per_rec = [flat[o:o + F].cpu().numpy() for o, F in c["recs"][:, :2]]
    unlinked_bits = tools.threshold_bits(flat, 0.5)[0].cpu().numpy()
    o1, o5, F = int(c["recs"][1, 0]), int(c["recs"][5, 0]), int(c["recs"][1, 1])
    assert (unlinked_bits[o1:o1 + F] != unlinked_bits[o5:o5 + F]).any()       # or a shared stream would show nothing
    for mode in LR.MODES:
        logits, bits = tools.window_frames_link(d_rows, c["tab"], c["wf"], c["recs"], ratio, CORE, context, c["links"], c["members"],
                                                mode, 0.5)
        assert logits.shape == bits.shape == (int(c["links"][:, 1].sum()),) and logits.dtype == torch.float32 and bits.dtype == torch.uint8
        want = np.concatenate([LR.link([per_rec[m] for m in c["members"][f:f + n]], mode) for _, _, f, n in c["links"]])
        got = logits.cpu().numpy()
        assert _same_bits(got, want), mode
        assert torch.equal(bits, tools.threshold_bits(logits, 0.5)[0]), mode
        near = LR.near_threshold(want)
        differ = bits.cpu().numpy() != LR.decide(want, 0.5)
        print(mode, "context", context, "frames", len(want), "near the threshold", int(near.sum()), "decided otherwise", int(differ.sum()))
        assert near.sum() <= 0.01 * len(want) and not differ[~near].any(), mode
        for g, (o, F, f, n) in enumerate(c["links"]):
            if n == 1:                                          # a group of one keeps its member's stitched logits
                assert _same_bits(got[o:o + F], per_rec[c["members"][f]]), (mode, g)
        # another threshold: the kernel's own argument, not a constant
        hi = tools.window_frames_link(d_rows, c["tab"], c["wf"], c["recs"], ratio, CORE, context, c["links"], c["members"], mode, 0.75)
        assert torch.equal(hi[0], logits) and torch.equal(hi[1], tools.threshold_bits(logits, 0.75)[0]) and not torch.equal(hi[1], bits)


@gpu
def test_a_group_alone_and_its_members_in_another_order():
    """The pair alone in a call of its own gives the bits it has in the batch; 'any' does not depend on the member order."""
    from sos_amd import tools
    c = _case()
    d_rows = torch.from_numpy(c["rows"]).cuda()
    F, o = int(c["links"][1, 1]), int(c["links"][1, 0])
    for mode in LR.MODES:
        batch = tools.window_frames_link(d_rows, c["tab"], c["wf"], c["recs"], SR / FPS, CORE, CONTEXT, c["links"], c["members"], mode)
        alone = tools.window_frames_link(d_rows, c["tab"], c["wf"], c["recs"], SR / FPS, CORE, CONTEXT, [(0, F, 0, 2)], [1, 5], mode)
        assert torch.equal(alone[0], batch[0][o:o + F]) and torch.equal(alone[1], batch[1][o:o + F])
    first = tools.window_frames_link(d_rows, c["tab"], c["wf"], c["recs"], SR / FPS, CORE, CONTEXT, [(0, F, 0, 2)], [1, 5], "any")
    swapped = tools.window_frames_link(d_rows, c["tab"], c["wf"], c["recs"], SR / FPS, CORE, CONTEXT, [(0, F, 0, 2)], [5, 1], "any")
    assert torch.equal(swapped[0], first[0]) and torch.equal(swapped[1], first[1])


SENTINEL, SPARE = -77.0, 16


def _spared(a, fill=0):
    a = np.asarray(a).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.full(SPARE, fill, a.dtype)])).cuda()


@gpu
def test_kernel_gives_no_work_to_what_a_device_entry_takes_outside_the_hosts_sizes():
    """The device rule of csrc/ragged.h: the host tables are correct, a DEVICE table differs in one entry.  The call succeeds,
    the group (or the frames) that need the entry are left as they were, everything else is what the unaltered call gives, and
    nothing past the buffers is written (spare elements behind every buffer keep a wrongly followed entry inside allocated
    memory)."""
    from sos_amd import _lib as L
    c = _case()
    tab, wf, recs, links, members = c["tab"], c["wf"], c["recs"], c["links"], c["members"]
    rat = np.full(len(NS), SR / FPS)
    W, stride, total, nrec = len(tab), c["rows"].shape[1], int(links[:, 1].sum()), len(NS)
    d_rows = _spared(c["rows"])
    assert members.tolist() == [0, 3, 6, 1, 5, 2, 4]

    def run(**dev):
        host = dict(tab=tab, wf=wf, recs=recs, rat=rat, links=links, members=members)
        d = {k: _spared(dev.get(k, v)) for k, v in host.items()}
        logits = torch.full((total + SPARE,), SENTINEL, device="cuda")
        bits = torch.full((total + SPARE,), 7, dtype=torch.uint8, device="cuda")
        rc = L.lib().sos_window_frames_link_f32(L.ptr(d_rows), W, stride, L.ptr(d["tab"]), tab.ctypes.data, L.ptr(d["wf"]), wf.ctypes.data,
                                                W, L.ptr(d["recs"]), recs.ctypes.data, L.ptr(d["rat"]), rat.ctypes.data, nrec, CORE,
                                                CONTEXT, L.ptr(d["links"]), links.ctypes.data, L.ptr(d["members"]), members.ctypes.data,
                                                len(links), 1, 0.5, L.ptr(logits), L.ptr(bits), L.stream_ptr())
        assert rc == 0, L.lib().sos_last_error().decode()
        return logits.cpu().numpy(), bits.cpu().numpy()

    def changed(a, i, col, value):
        a = a.copy()
        if a.ndim == 1:
            a[i] = value
        else:
            a[i, col] = value
        return a

    base, base_bits = run()
    assert not (base[:total] == SENTINEL).any() and (base[total:] == SENTINEL).all()
    assert (base_bits[:total] <= 1).all() and (base_bits[total:] == 7).all()
    for group, dev in ((1, dict(links=changed(links, 1, 0, total))), (1, dict(links=changed(links, 1, 1, total))),
                       (2, dict(links=changed(links, 2, 0, -1))), (0, dict(links=changed(links, 0, 3, len(members) + 1))),
                       (0, dict(links=changed(links, 0, 3, 0))), (3, dict(links=changed(links, 3, 2, len(members)))),
                       (1, dict(links=changed(links, 1, 2, -1))), (0, dict(members=changed(members, 1, 0, nrec))),
                       (1, dict(members=changed(members, 4, 0, -1))), (1, dict(recs=changed(recs, 5, 1, recs[5, 1] - 1))),
                       (1, dict(recs=changed(recs, 1, 3, 0))), (0, dict(recs=changed(recs, 6, 2, W))),
                       (3, dict(recs=changed(recs, 4, 3, W + 1))), (0, dict(rat=changed(rat, 3, 0, -1.0))),
                       (1, dict(rat=changed(rat, 5, 0, np.nan)))):
        got, got_bits = run(**dev)
        lo, hi = int(links[group, 0]), int(links[group, 0] + links[group, 1])
        assert (got[lo:hi] == SENTINEL).all() and (got_bits[lo:hi] == 7).all(), (group, dev)
        assert _same_bits(got[:lo], base[:lo]) and _same_bits(got[hi:total], base[hi:total]), (group, dev)
        assert np.array_equal(got_bits[:lo], base_bits[:lo]) and np.array_equal(got_bits[hi:total], base_bits[hi:total]), (group, dev)
        assert (got[total:] == SENTINEL).all() and (got_bits[total:] == 7).all(), (group, dev)
    # a window's entry (the middle window of recording 5, a member of the pair): only the frames that need it are left alone
    w = int(recs[5, 2]) + 1
    lo, hi = int(links[1, 0]), int(links[1, 0] + links[1, 1])
    for dev in (dict(tab=changed(tab, w, 7, W)), dict(tab=changed(tab, w, 7, -1)), dict(wf=changed(wf, w, 0, stride + 1)),
                dict(wf=changed(wf, w, 0, 0))):
        got, got_bits = run(**dev)
        left = got[lo:hi] == SENTINEL
        assert 20 <= left.sum() < hi - lo and np.array_equal(left, got_bits[lo:hi] == 7)
        assert _same_bits(got[lo:hi][~left], base[lo:hi][~left]) and _same_bits(got[:lo], base[:lo]) and _same_bits(got[hi:total], base[hi:total])
        assert (got[total:] == SENTINEL).all() and (got_bits[total:] == 7).all()


# ---- end to end

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
def clips():
    """Two three-window recordings of one length and a short one: synthetic noisy speech, on the GPU.  Never modified."""
    from sos_amd.dataset import synth_batch

    def wave(seed, n):
        parts = synth_batch(seed, (n + 27999) // 28000)["mixed"]
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(list(parts))[:n])).cuda()

    return [wave(710, N_LONG), wave(711, N_LONG), wave(720, 14000 + 157)]


LINK = [0, 0, None]


class _mode:
    def __init__(self, precision):
        self.precision = precision

    def __enter__(self):
        sos_amd.set_precision(self.precision)

    def __exit__(self, *exc):
        sos_amd.set_precision("bf16")


@pytest.fixture(scope="module")
def runs(nets, clips):
    """Per precision, computed once and left unchanged: the unlinked detect_long, and per link mode the linked detect_long and
    denoise_long(stitch_bits=True, link=) with return_all."""
    from sos_amd import pipeline
    det, jm = nets
    res = {}
    for precision in PRECISIONS:
        with _mode(precision):
            e = dict(unlinked=pipeline.detect_long(det, clips, **SECONDS),
                     plain=pipeline.denoise_long(det, jm, clips, stitch_bits=True, **SECONDS))
            for mode in LR.MODES:
                e[mode] = dict(pairs=pipeline.detect_long(det, clips, link=LINK, link_mode=mode, **SECONDS),
                               long=pipeline.denoise_long(det, jm, clips, stitch_bits=True, link=LINK, link_mode=mode, return_all=True,
                                                          **SECONDS))
        res[precision] = e
    return res


@gpu
@pytest.mark.parametrize("mode", LR.MODES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_detect_long_gives_both_members_the_groups_one_stream(runs, precision, mode):
    from sos_amd import pipeline, tools
    unlinked, pairs = runs[precision]["unlinked"], runs[precision][mode]["pairs"]
    F = pipeline.n_video_frames(N_LONG)
    assert pairs[0][0] is pairs[1][0] and pairs[0][1] is pairs[1][1]             # the same tensors, not copies
    logits, bits = pairs[0]
    assert logits.shape == bits.shape == (F,) and bits.dtype == torch.uint8
    want = LR.link([unlinked[0][0].cpu().numpy(), unlinked[1][0].cpu().numpy()], mode)
    assert _same_bits(logits.cpu().numpy(), want)
    assert torch.equal(bits, tools.threshold_bits(logits, pipeline.SIGMOID_THRESHOLD)[0])
    assert torch.equal(pairs[2][0], unlinked[2][0]) and torch.equal(pairs[2][1], unlinked[2][1])
    print(precision, mode, "frames", F, "speech in channel 0 / 1 / shared", int(unlinked[0][1].sum()), int(unlinked[1][1].sum()), int(bits.sum()))
    if mode == "any":                                                             # speech wherever a member has speech
        assert bool((bits >= torch.maximum(unlinked[0][1], unlinked[1][1])).all())


@gpu
@pytest.mark.parametrize("mode", LR.MODES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_denoise_long_is_the_bits_path_on_the_groups_streams(nets, clips, runs, precision, mode):
    from sos_amd import pipeline
    _, jm = nets
    pairs, (outs, extra) = runs[precision][mode]["pairs"], runs[precision][mode]["long"]
    with _mode(precision):
        want = pipeline.denoise_long(None, jm, clips, bits=[b for _, b in pairs], fps=FPS, **SECONDS)
    for r, (o, w, e, c) in enumerate(zip(outs, want, extra, clips)):
        assert o.shape == (HOP * (c.numel() // HOP),) and torch.equal(o, w) and bool(torch.isfinite(o).all()), r
        assert torch.equal(e["logits"], pairs[r][0]) and torch.equal(e["bits"], pairs[r][1]), r
        assert sorted(e) == ["bits", "logits", "mask", "plan"]
    assert torch.equal(extra[0]["mask"], extra[1]["mask"])                        # one stream, one length: one mask


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_groups_of_one_are_plain_stitch_bits_and_signals_work(nets, clips, runs, precision):
    from sos_amd import pipeline
    det, jm = nets
    with _mode(precision):
        for mode in LR.MODES:
            got = pipeline.denoise_long(det, jm, clips, stitch_bits=True, link=[None, None, None], link_mode=mode, **SECONDS)
            assert all(torch.equal(a, b) for a, b in zip(got, runs[precision]["plain"])), mode
        outs, extra = pipeline.denoise_long(det, jm, clips, stitch_bits=True, link=LINK, signals=True, **SECONDS)
    assert all(torch.equal(a, b) for a, b in zip(outs, runs[precision]["any"]["long"][0]))
    assert all(sorted(e) == ["noise_intervals", "noisy_input", "predicted_full_noise"] and e["noisy_input"].shape == o.shape
               for e, o in zip(extra, outs))


@gpu
def test_link_raises_before_any_launch_and_nothing_synchronises(nets, clips):
    from sos_amd import pipeline
    det, jm = nets
    with _mode("bf16x3"):
        pipeline.detect_long(det, clips, link=LINK, **SECONDS)                    # plans, tables and workspaces are built
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(ValueError, match="stitch_bits=True"):
                pipeline.denoise_long(det, jm, clips, link=LINK, **SECONDS)
            with pytest.raises(ValueError, match="link_mode"):
                pipeline.detect_long(det, clips, link=LINK, link_mode="max", **SECONDS)
            with pytest.raises(ValueError, match="recording 2 has"):
                pipeline.detect_long(det, clips, link=[0, 0, 0], **SECONDS)
            with pytest.raises(ValueError, match="one group id"):
                pipeline.detect_long(det, clips, link=[0, 0], **SECONDS)
            pairs = pipeline.detect_long(det, clips, link=LINK, **SECONDS)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    assert pairs[0][0] is pairs[1][0] and bool(torch.isfinite(pairs[0][0]).all())
