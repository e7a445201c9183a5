"""sos_window_stage_f32 / sos_window_stitch_f32 (csrc/ragged_window.hip) and pipeline.denoise_long: long recordings cut into
overlapping windows, run as ragged clips and cross-faded back.  The reference is tests/window_reference.py (float64, independent
of the package's window_plan).  The kernels know nothing of the hop, so their tests use tiny cores; copies are compared bit for
bit, blended samples within 4 * 2^-24 * max(|a|, |b|): one rounding each for w and 1 - w, two products and a sum (an FMA
contraction drops one of them)."""
import numpy as np
import pytest
import torch

import sos_amd
import window_reference as R
from oracle import nets as onet

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
SPARE = 16
HOP = 158


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _tiny(ns, core=8, context=4):
    """Plan and table of recordings of `ns` samples at hop 1 (output length = length)."""
    wins = R.plan(ns, core, context, hop=1, min_frames=1)
    return wins, R.table(wins, ns, hop=1)


def _subtable(tab, idx, out_shift=0):
    """Rows `idx` of a table, in that order, as a table of their own: neighbours renumbered, outputs moved by -out_shift."""
    new = {int(w): i for i, w in enumerate(idx)}
    sub = tab[np.asarray(idx)].copy()
    sub[:, 3] -= out_shift
    for col in (8, 9):
        sub[:, col] = [new[int(v)] if v >= 0 else -1 for v in sub[:, col]]
    return np.ascontiguousarray(sub)


# ---- stage

@pytest.mark.parametrize("stride", [20, 23], ids=["stride%4=0", "stride%4=3"])
def test_stage_rows_are_the_slices_and_zero_beyond(stride):
    from sos_amd import tools
    ns = [1, 5, 4097, 3 * 8 + 7]
    wins, tab = _tiny(ns)
    assert len(wins) == 1 + 1 + 512 + 3 and max(w.samples for w in wins) == 19
    flat = np.random.default_rng(5).standard_normal(sum(ns)).astype(np.float32)
    assert any(o % 4 for o in tab[:, 1]) and any(o % 4 == 0 for o in tab[:, 1])          # both access paths
    assert tab[-1, 1] + tab[-1, 2] == len(flat)                                          # the last window ends at the last float
    rows = tools.window_stage(torch.from_numpy(flat).cuda(), tab, stride).cpu().numpy()
    assert rows.shape == (len(wins), stride)
    for w, (off, m) in enumerate(tab[:, 1:3]):
        assert _same_bits(rows[w, :m], flat[off:off + m]) and not rows[w, m:].any(), w


def test_stage_65535_windows():
    """Three recordings with 70 000 windows between them, cut to the 65 535 a launch takes (grid.y)."""
    from sos_amd import tools
    ns = [8 * 30000 + 3, 8 * 25000 + 5, 8 * 15000 + 1]
    wins, full = _tiny(ns)
    assert len(wins) == 70000
    tab = np.ascontiguousarray(full[:65535])
    flat = np.random.default_rng(6).standard_normal(sum(ns)).astype(np.float32)
    d_flat = torch.from_numpy(flat).cuda()
    rows = tools.window_stage(d_flat, tab, 20).cpu().numpy()
    j = np.arange(20)[None, :]
    valid = j < tab[:, 2:3]
    want = np.where(valid, flat[np.minimum(tab[:, 1:2] + j, len(flat) - 1)], np.float32(0))
    assert _same_bits(rows, want)
    with pytest.raises(RuntimeError, match=r"rc=-22.*65535 windows"):
        tools.window_stage(d_flat, full[:65536], 20)


# ---- stitch

def _stitch_case(ns, core, context, seed, pad=3):
    """Random rows (also beyond the windows' samples: never read) for the plan of `ns`, and the f64 stitch per recording."""
    wins, tab = _tiny(ns, core, context)
    stride = max(w.samples for w in wins) + pad
    rows = np.random.default_rng(seed).standard_normal((len(wins), stride)).astype(np.float32)
    per_rec = []
    for r in range(len(ns)):
        idx = [i for i, w in enumerate(wins) if w.recording == r]
        mine, rr = [wins[i] for i in idx], [rows[i, :wins[i].samples] for i in idx]
        out, blended = R.stitch(mine, rr, context)
        per_rec.append((idx, out, blended, R.stitch_bound(mine, rr, context)))
    return wins, tab, rows, per_rec


def _check_stitched(got, per_rec, ns):
    pos = 0
    for r, (idx, out, blended, bound) in enumerate(per_rec):
        g = got[pos:pos + ns[r]]
        assert _same_bits(g[~blended], out[~blended].astype(np.float32)), r           # f64 of an f32 copy: exact
        err = np.abs(g.astype(np.float64) - out)
        assert np.all(err[blended] <= bound[blended]), (r, float((err[blended] / np.maximum(bound[blended], 1e-300)).max()))
        pos += ns[r]
    assert pos == len(got)


@pytest.mark.parametrize("ns,core,context", [
    ([31, 5, 4097, 16, 100], 8, 4),                   # core = 2 context: an inner core is all overlap
    ([31, 5, 4097, 16, 100], 8, 0),                   # a plain cut
    ([5000, 2999, 12345, 2000], 1000, 300),           # several workgroups' worth per core, every alignment of the three rows
    ([5000, 2999, 12345, 2000], 1001, 1),
], ids=["core8-context4", "core8-cut", "core1000-context300", "core1001-context1"])
def test_stitch_copies_outside_and_blends_inside_the_overlaps(ns, core, context):
    from sos_amd import tools
    wins, tab, rows, per_rec = _stitch_case(ns, core, context, seed=core + context)
    d_rows = torch.from_numpy(rows).cuda()
    got = tools.window_stitch(d_rows, tab, context).cpu().numpy()
    assert got.shape == (sum(ns),)
    _check_stitched(got, per_rec, ns)
    if context == 0:                                  # an exact cut at the core boundaries, whatever the rows hold elsewhere
        want = np.concatenate([rows[i, w.core_start - w.start:w.core_end - w.start] for i, w in enumerate(wins)])
        assert _same_bits(got, want)
    else:
        assert sum(int(b.sum()) for _, _, b, _ in per_rec) == 2 * context * sum(len(i) - 1 for i, _, _, _ in per_rec) > 0


def test_stitch_same_bits_alone_in_a_batch_and_permuted():
    from sos_amd import tools
    ns = [5001, 2999, 12345, 2000]                    # outputs start at 0, 5001, 8000, 20345: 0, 1, 0, 1 mod 4
    wins, tab, rows, per_rec = _stitch_case(ns, 1000, 300, seed=9)
    d_rows = torch.from_numpy(rows).cuda()
    batch = tools.window_stitch(d_rows, tab, 300).cpu().numpy()
    perm = np.random.default_rng(10).permutation(len(wins))
    assert _same_bits(tools.window_stitch(d_rows, _subtable(tab, perm), 300).cpu().numpy(), batch)
    starts = np.cumsum(ns) - ns
    for r, (idx, _, _, _) in enumerate(per_rec):
        alone = tools.window_stitch(d_rows, _subtable(tab, idx, starts[r]), 300).cpu().numpy()
        assert _same_bits(alone, batch[starts[r]:starts[r] + ns[r]]), r
    # the rows in another order and at another stride: row indices are the table's business
    order = np.random.default_rng(11).permutation(len(wins))
    moved = np.zeros((len(wins), rows.shape[1] + 1), np.float32)
    moved[order, :-1] = rows
    tab2 = tab.copy()
    tab2[:, 7] = order
    assert _same_bits(tools.window_stitch(torch.from_numpy(moved).cuda(), tab2, 300).cpu().numpy(), batch)


# ---- refusals on the host, and the device rule

def _raw(name, *args):
    from sos_amd import _lib as L
    rc = getattr(L.lib(), name)(*args, L.stream_ptr())
    return rc, L.lib().sos_last_error().decode()


def test_host_refusals_name_the_window():
    from sos_amd import _lib as L
    ns = [31, 5, 100]
    wins, tab = _tiny(ns)
    W, stride, total = len(wins), 24, sum(ns)
    flat = torch.zeros(total, device="cuda")
    rows = torch.zeros((W, stride), device="cuda")
    out = torch.zeros(total, device="cuda")
    d_tab = torch.from_numpy(tab).cuda()

    def stage(t=tab, x=flat, total=total, nwin=W, stride=stride, dev=d_tab, rows=rows):
        t = np.ascontiguousarray(t)
        return _raw("sos_window_stage_f32", L.ptr(x), total, L.ptr(dev), t.ctypes.data, nwin, stride, L.ptr(rows))

    def stitch(t=tab, rows=rows, n_rows=W, stride=stride, nwin=W, context=4, dev=d_tab, out=out):
        t = np.ascontiguousarray(t)
        return _raw("sos_window_stitch_f32", L.ptr(rows), n_rows, stride, L.ptr(dev), t.ctypes.data, nwin, context, L.ptr(out))

    def changed(w, col, value):
        t = tab.copy()
        t[w, col] = value
        return t

    assert stage()[0] == 0 and stitch()[0] == 0
    for rc, msg in (stage(x=None), stage(rows=None), stage(dev=None), stitch(rows=None), stitch(out=None), stitch(dev=None)):
        assert rc == -22 and "null pointer" in msg, msg
    from sos_amd import _lib
    assert _lib.lib().sos_window_stage_f32(L.ptr(flat), total, L.ptr(d_tab), None, W, stride, L.ptr(rows), L.stream_ptr()) == -22
    assert _lib.lib().sos_window_stitch_f32(L.ptr(rows), W, stride, L.ptr(d_tab), None, W, 4, L.ptr(out), L.stream_ptr()) == -22
    for call in (stage, stitch):
        for kw in (dict(nwin=0), dict(nwin=65536), dict(stride=0)):
            rc, msg = call(**kw)
            assert rc == -22 and "bad args" in msg, (kw, msg)
        rc, msg = call(t=changed(2, 2, stride + 1))                       # samples > stride
        assert rc == -22 and "window 2 " in msg and "stride" in msg, msg
    # an entry outside `total`: by its offset, by its length, and a negative one
    for t in (changed(3, 1, total - tab[3, 2] + 1), changed(1, 1, -1), changed(W - 1, 2, tab[W - 1, 2] + 1)):
        rc, msg = stage(t=t)
        assert rc == -22 and "window %d " % int(np.flatnonzero((t != tab).any(axis=1))[0]) in msg and "outside" in msg, msg
    assert stage(total=total - 1)[0] == -22 and "window %d " % (W - 1) in stage(total=total - 1)[1]
    for what, t, kw in (("a row outside n_rows", changed(4, 7, W), {}), ("a negative row", changed(4, 7, -1), {}),
                        ("fewer rows than the table names", tab, dict(n_rows=W - 1)),
                        ("an output past the summed length", changed(W - 1, 3, tab[W - 1, 3] + 1), {}),
                        ("a core outside the window", changed(1, 6, tab[1, 4] + 1), {}),
                        ("a neighbour that does not exist", changed(1, 9, W), {}),
                        ("a neighbour of another recording", changed(1, 9, W - 1), {}),
                        ("a context that is not less than the window", tab, dict(context=12)),
                        ("a context longer than half an inner core", tab, dict(context=5))):
        rc, msg = stitch(t=t, **kw)
        assert rc == -22 and "window" in msg and any("window %d " % w in msg for w in range(W)), (what, msg)
    rc, msg = stitch(context=-1)
    assert rc == -22 and "context" in msg, msg
    assert stitch(t=changed(4, 7, W))[1].startswith("sos_window_stitch_f32: window 4 ")


def _spared(a, fill=0):
    a = np.asarray(a).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.full(SPARE, fill, a.dtype)])).cuda()


def test_kernels_skip_a_device_entry_that_leaves_the_hosts_sizes():
    """The device rule: the host table is correct, the DEVICE table differs in one entry.  The calls succeed, that window's row
    (stage) or core (stitch) is left as it was, everything else is what the unaltered call gives, nothing past the buffers is
    written (spare elements behind every buffer keep a wrongly followed entry inside allocated memory)."""
    from sos_amd import _lib as L
    ns = [31, 5, 100]
    wins, tab = _tiny(ns)
    W, stride, total = len(wins), 24, sum(ns)
    rng = np.random.default_rng(12)
    flat, rows_in = _spared(rng.standard_normal(total).astype(np.float32)), _spared(rng.standard_normal((W, stride)).astype(np.float32))

    def stage(d_tab):
        rows = torch.full((W * stride + SPARE,), SENTINEL, device="cuda")
        assert L.lib().sos_window_stage_f32(L.ptr(flat), total, L.ptr(d_tab), tab.ctypes.data, W, stride, L.ptr(rows), L.stream_ptr()) == 0
        return rows.cpu().numpy()

    def stitch(d_tab):
        out = torch.full((total + SPARE,), SENTINEL, device="cuda")
        assert L.lib().sos_window_stitch_f32(L.ptr(rows_in), W, stride, L.ptr(d_tab), tab.ctypes.data, W, 4, L.ptr(out), L.stream_ptr()) == 0
        return out.cpu().numpy()

    base_rows, base_out = stage(torch.from_numpy(tab).cuda()), stitch(torch.from_numpy(tab).cuda())
    assert not (base_rows[:-SPARE] == SENTINEL).any() and not (base_out[:-SPARE] == SENTINEL).any()
    for w, col, value in ((2, 1, total - tab[2, 2] + 1), (2, 2, stride + 1), (3, 1, -1)):
        d_tab = torch.from_numpy(tab).cuda()
        d_tab[w, col] = int(value)
        got = stage(d_tab)
        assert (got[w * stride:(w + 1) * stride] == SENTINEL).all() and (got[-SPARE:] == SENTINEL).all(), (col, value)
        assert _same_bits(got[:w * stride], base_rows[:w * stride]) and _same_bits(got[(w + 1) * stride:], base_rows[(w + 1) * stride:])
    # window 3 is a recording of its own (no window reads its entry as a neighbour's); window 2 is the last of three: its
    # `previous` is read by itself only
    for w, col, value in ((3, 7, W), (3, 3, total), (3, 5, tab[3, 5] + 1), (3, 2, stride + 1), (3, 6, 1), (2, 8, W), (2, 8, 4)):
        lo, hi = int(tab[w, 3] + tab[w, 4] - tab[w, 6]), int(tab[w, 3] + tab[w, 5] - tab[w, 6])
        d_tab = torch.from_numpy(tab).cuda()
        d_tab[w, col] = int(value)
        got = stitch(d_tab)
        assert (got[lo:hi] == SENTINEL).all() and (got[-SPARE:] == SENTINEL).all(), (w, col, value)
        assert _same_bits(got[:lo], base_out[:lo]) and _same_bits(got[hi:total], base_out[hi:total]), (w, col, value)


# ---- end to end: the closed-form networks of tests/test_gpu_pipeline.py

CORE, CONTEXT = 80 * HOP, 8 * HOP
SECONDS = dict(window_seconds=CORE / 14000, context_seconds=CONTEXT / 14000)
N_ONE, N_LONG = 150 * HOP + 31, 3 * CORE + 5 * HOP + 77


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


def _check_against_rows(got, wins, rows):
    """`got` (the stitched output of one recording) against the f64 stitch of its windows' result rows."""
    want, blended = R.stitch(wins, rows, CONTEXT)
    bound = R.stitch_bound(wins, rows, CONTEXT)
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    assert _same_bits(got[~blended], want[~blended].astype(np.float32))
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err[blended] <= bound[blended]), float((err[blended] / np.maximum(bound[blended], 1e-300)).max())
    assert blended.sum() == 2 * CONTEXT * (len(wins) - 1)


@pytest.mark.parametrize("precision", ["bf16x3", "fp16"])
def test_a_recording_of_one_window_is_denoise_ragged(nets, waves, precision):
    from sos_amd import pipeline
    det, jm = nets
    assert len(R.plan([N_ONE], CORE, CONTEXT)) == 1
    with _mode(precision):
        got, extra = pipeline.denoise_long(det, jm, [waves[0]], return_all=True, **SECONDS)
        want, wextra = pipeline.denoise_ragged(det, jm, [waves[0]], return_all=True)
    assert got[0].shape == (150 * HOP,) and torch.equal(got[0], want[0])
    assert np.array_equal(extra[0]["plan"], R.table(R.plan([N_ONE], CORE, CONTEXT), [N_ONE]))
    assert torch.equal(extra[0]["windows"][0]["bits"], wextra[0]["bits"]) and torch.equal(extra[0]["windows"][0]["logits"], wextra[0]["logits"])


@pytest.mark.parametrize("max_batch", [256, 2], ids=["one-group", "two-groups"])
@pytest.mark.parametrize("precision", ["bf16x3", "fp16"])
def test_three_windows_are_the_stitched_ragged_clips(nets, waves, precision, max_batch):
    """denoise_ragged of the three windows cut on the host groups them as denoise_long does (same lengths, same limits), so the
    rows coincide bit for bit; max_batch = 2 puts the windows of the one recording into two groups."""
    from sos_amd import pipeline
    det, jm = nets
    long = waves[1]
    wins = R.plan([N_LONG], CORE, CONTEXT)
    assert len(wins) == 3 and wins[-1].core_end == 3 * CORE + 5 * HOP
    with _mode(precision):
        got, extra = pipeline.denoise_long(det, jm, [long], max_batch=max_batch, return_all=True, **SECONDS)
        again = pipeline.denoise_long(det, jm, [long], max_batch=max_batch, **SECONDS)
        rows, wextra = pipeline.denoise_ragged(det, jm, [long[w.start:w.start + w.samples] for w in wins], max_batch=max_batch, return_all=True)
    assert len(got) == 1 and got[0].shape == (3 * CORE + 5 * HOP,)
    assert torch.equal(got[0], again[0])                                   # a repeated call is bit-identical
    assert [tuple(r.shape) for r in rows] == [(HOP * (w.samples // HOP),) for w in wins]
    _check_against_rows(got[0], wins, [r.cpu().numpy() for r in rows])
    plan = extra[0]["plan"]
    assert np.array_equal(np.delete(plan, 7, axis=1), np.delete(R.table(wins, [N_LONG]), 7, axis=1)) and sorted(plan[:, 7]) == [0, 1, 2]
    for k in range(3):
        assert torch.equal(extra[0]["windows"][k]["bits"], wextra[k]["bits"])
        assert extra[0]["windows"][k]["bits"].shape == (pipeline.n_video_frames(wins[k].samples),)


@pytest.mark.parametrize("precision", ["bf16x3", "fp16"])
def test_a_mixed_list_returns_in_input_order(nets, waves, precision):
    """[short, long, short]: with one window per group (max_batch = 1) every window runs exactly as in a list of its own, so each
    entry equals its stand-alone result bit for bit; with the default grouping lengths, order and finiteness are checked."""
    from sos_amd import pipeline
    det, jm = nets
    clips = [waves[0], waves[1], waves[2]]
    with _mode(precision):
        got = pipeline.denoise_long(det, jm, clips, max_batch=1, **SECONDS)
        alone = [pipeline.denoise_long(det, jm, [c], max_batch=1, **SECONDS)[0] for c in clips]
        grouped = pipeline.denoise_long(det, jm, clips, **SECONDS)
    for g, a, gg, c in zip(got, alone, grouped, clips):
        assert g.shape == gg.shape == (HOP * (c.numel() // HOP),) and torch.equal(g, a) and bool(torch.isfinite(gg).all())


@pytest.mark.parametrize("precision", ["bf16x3", "fp16"])
def test_given_bits_are_masked_at_full_length_and_windowed(nets, waves, precision):
    """bits= at 25 frames per second: the sample mask is that of the whole recording, and the output is the stitch of the
    denoiser's rows on the host-cut windows of the recording and of its full-length noise-interval signal."""
    from sos_amd import pipeline, tools
    _, jm = nets
    long = waves[1]
    bits = torch.from_numpy(np.random.default_rng(13).integers(0, 2, pipeline.n_video_frames(N_LONG, 14000, 25)).astype(np.uint8)).cuda()
    wins = R.plan([N_LONG], CORE, CONTEXT)
    with _mode(precision):
        got, extra = pipeline.denoise_long(None, jm, [long], fps=25, bits=[bits], return_all=True, **SECONDS)
        mask, noise = tools.bits_to_mask_batch(bits[None], 14000 / 25, N_LONG, long[None])
        # the group denoise_long forms of these windows: longest first, all three in one group
        order = pipeline._length_groups([w.samples for w in wins], 256, 65536)
        assert len(order) == 1
        ms = [wins[i].samples for i in order[0]]
        wave, masked = torch.zeros((3, max(ms)), device="cuda"), torch.zeros((3, max(ms)), device="cuda")
        for k, i in enumerate(order[0]):
            w = wins[i]
            wave[k, :w.samples], masked[k, :w.samples] = long[w.start:w.start + w.samples], noise[0, w.start:w.start + w.samples]
        rag = pipeline._group_geometry(ms, wave.device, 14000, 30.0, nv=[1] * 3)
        y = pipeline._denoise_group_staged(jm, wave, masked, rag).cpu().numpy()
    assert torch.equal(extra[0]["mask"], mask[0]) and torch.equal(extra[0]["bits"], bits)
    assert 0 < float(mask.sum()) < N_LONG
    rows = [None] * 3
    for k, i in enumerate(order[0]):
        rows[i] = y[k, :HOP * (wins[i].samples // HOP)]
    _check_against_rows(got[0], wins, rows)


def test_denoise_long_refuses_before_any_launch(nets, waves):
    from sos_amd import pipeline
    det, jm = nets
    short = torch.zeros(64 * HOP - 1, device="cuda")
    with pytest.raises(ValueError, match="recording 1"):
        pipeline.denoise_long(det, jm, [waves[0], short], **SECONDS)
    with pytest.raises(ValueError):
        pipeline.denoise_long(det, jm, [waves[0]], window_seconds=1.0, context_seconds=0.6)
    with pytest.raises(ValueError):
        pipeline.denoise_long(det, jm, [waves[0][None]], **SECONDS)
    assert pipeline.denoise_long(det, jm, [], **SECONDS) == []
