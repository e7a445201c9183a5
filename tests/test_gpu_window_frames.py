"""sos_window_frames_stitch_f32 (csrc/ragged_window.hip): the windows' frame logits stitched into one logit stream per recording,
against tests/frames_reference.py (float64, independent of the package).  Kernel level: no networks, random logit rows.  Copies
are compared bit for bit; blended frames within the reference's bound 4 * 2^-24 * max(|a|, |b|)."""
import numpy as np
import pytest
import torch

import frames_reference as FR
import window_reference as R

pytestmark = pytest.mark.gpu

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
SR = 14000
NS = [150 * HOP + 31, 3 * CORE + 5 * HOP + 77, 2 * CORE, 2 * CORE - 1, 5 * CORE + HOP - 1]
SENTINEL = -77.0
SPARE = 16


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _case(ns, fps, context=CONTEXT, seed=3, pad=3):
    """Plan, table, per-window frame counts, random rows (also beyond a window's frames: never read), the recordings' table and
    the float64 stitch of every recording."""
    wins = R.plan(ns, CORE, CONTEXT)
    tab = R.table(wins, ns)
    per_rec, wf, recs, foff = [], [], [], 0
    for r in range(len(ns)):
        idx = [i for i, w in enumerate(wins) if w.recording == r]
        wf += FR.window_frames([wins[i] for i in idx], SR, fps)
        F = FR.n_video_frames(ns[r], SR, fps)
        recs.append((foff, F, idx[0], len(idx)))
        foff += F
        per_rec.append(idx)
    rows = np.random.default_rng(seed).standard_normal((len(wins), max(wf) + pad)).astype(np.float32)
    refs = [FR.stitch([wins[i] for i in idx], [rows[i, :wf[i]] for i in idx], SR, fps, CORE, context) for idx in per_rec]
    return tab, np.asarray(wf, np.int64), rows, np.asarray(recs, np.int64), refs


def _check(got, recs, refs):
    assert got.shape == (int(recs[:, 1].sum()),)
    for (foff, F, _, _), st in zip(recs, refs):
        g = got[foff:foff + F]
        assert _same_bits(g[~st.blended], st.out[~st.blended].astype(np.float32))         # f64 of an f32 copy: exact
        err = np.abs(g.astype(np.float64) - st.out)
        print("frames", F, "blended", int(st.blended.sum()), "clamped", st.clamped,
              "max err / bound %.3f" % float((err[st.blended] / np.maximum(st.bound[st.blended], 1e-300)).max() if st.blended.any() else 0))
        assert np.all(err <= st.bound)


@pytest.mark.parametrize("fps", [30.0, 25.0, 29.97])
def test_frames_are_copied_outside_and_blended_inside_the_zones(fps):
    from sos_amd import tools
    tab, wf, rows, recs, refs = _case(NS, fps)
    assert [int(k) for k in recs[:, 3]] == [1, 3, 2, 1, 5]
    assert all(5 <= int(st.blended.sum()) <= 23 for st in refs if len(st.out) and st.owner[-1] > 0)
    if fps != 30.0:
        assert 1 <= sum(st.clamped for st in refs) <= 4                                   # the clamp is exercised
    got = tools.window_frames_stitch(torch.from_numpy(rows).cuda(), tab, wf, recs, SR / fps, CORE, CONTEXT).cpu().numpy()
    _check(got, recs, refs)
    for (foff, F, first, K) in recs[recs[:, 3] == 1]:                                     # one window: its own logits
        assert _same_bits(got[foff:foff + F], rows[first, :F])


@pytest.mark.parametrize("fps", [30.0, 29.97])
def test_context_zero_is_a_pure_copy(fps):
    from sos_amd import tools
    tab, wf, rows, recs, refs = _case(NS, fps, context=0)
    got = tools.window_frames_stitch(torch.from_numpy(rows).cuda(), tab, wf, recs, SR / fps, CORE, 0).cpu().numpy()
    want = np.concatenate([rows[first + st.owner, st.index] for (_, _, first, _), st in zip(recs, refs)])
    assert not any(st.blended.any() for st in refs) and _same_bits(got, want)


def test_same_bits_alone_in_a_batch_permuted_and_with_rows_in_another_order():
    from sos_amd import tools
    fps = 29.97
    tab, wf, rows, recs, refs = _case(NS, fps)
    d_rows = torch.from_numpy(rows).cuda()
    batch = tools.window_frames_stitch(d_rows, tab, wf, recs, SR / fps, CORE, CONTEXT).cpu().numpy()
    # every recording alone: its windows as a table of their own, its output at offset 0
    for r, (foff, F, first, K) in enumerate(recs):
        alone = tools.window_frames_stitch(d_rows, tab[first:first + K], wf[first:first + K], [(0, F, 0, K)], SR / fps, CORE, CONTEXT)
        assert _same_bits(alone.cpu().numpy(), batch[foff:foff + F]), r
    # the recordings permuted: their windows stay together and in order, the outputs move
    perm = [3, 1, 4, 0, 2]
    tab2 = np.concatenate([tab[recs[r, 2]:recs[r, 2] + recs[r, 3]] for r in perm])
    wf2 = np.concatenate([wf[recs[r, 2]:recs[r, 2] + recs[r, 3]] for r in perm])
    counts, frames = recs[perm, 3], recs[perm, 1]
    recs2 = np.stack([np.cumsum(frames) - frames, frames, np.cumsum(counts) - counts, counts], axis=1)
    got = tools.window_frames_stitch(d_rows, tab2, wf2, recs2, SR / fps, CORE, CONTEXT).cpu().numpy()
    for (foff2, F, _, _), r in zip(recs2, perm):
        assert _same_bits(got[foff2:foff2 + F], batch[recs[r, 0]:recs[r, 0] + F]), r
    # the rows in another order and at another stride: row indices are the table's business
    order = np.random.default_rng(11).permutation(len(tab))
    moved = np.zeros((len(tab), rows.shape[1] + 1), np.float32)
    moved[order, :-1] = rows
    tab3 = tab.copy()
    tab3[:, 7] = order
    assert _same_bits(tools.window_frames_stitch(torch.from_numpy(moved).cuda(), tab3, wf, recs, SR / fps, CORE, CONTEXT).cpu().numpy(), batch)


def test_one_ratio_per_recording():
    from sos_amd import tools
    ns, rates = [NS[1], NS[2]], [25.0, 30.0]
    parts = [_case([n], f, seed=20 + i) for i, (n, f) in enumerate(zip(ns, rates))]
    K0, F0 = len(parts[0][0]), int(parts[0][3][0, 1])
    stride = max(p[2].shape[1] for p in parts)
    rows = np.zeros((K0 + len(parts[1][0]), stride), np.float32)
    rows[:K0, :parts[0][2].shape[1]], rows[K0:, :parts[1][2].shape[1]] = parts[0][2], parts[1][2]
    tab = np.concatenate([parts[0][0], parts[1][0]])
    tab[K0:, 7] += K0
    recs = np.asarray([(0, F0, 0, K0), (F0, parts[1][3][0, 1], K0, len(parts[1][0]))], np.int64)
    got = tools.window_frames_stitch(torch.from_numpy(rows).cuda(), tab, np.concatenate([parts[0][1], parts[1][1]]), recs,
                                     [SR / f for f in rates], CORE, CONTEXT).cpu().numpy()
    _check(got, recs, [parts[0][4][0], parts[1][4][0]])


def _raw(*args):
    from sos_amd import _lib as L
    rc = L.lib().sos_window_frames_stitch_f32(*args, L.stream_ptr())
    return rc, L.lib().sos_last_error().decode()


def test_host_refusals_name_the_window_or_the_recording():
    from sos_amd import _lib as L
    fps = 30.0
    tab, wf, rows, recs, _ = _case(NS[:3], fps)
    rat = np.full(3, SR / fps)
    W, stride, total = len(tab), rows.shape[1], int(recs[:, 1].sum())
    d_rows, out = torch.from_numpy(rows).cuda(), torch.zeros(total, device="cuda")
    d_tab, d_wf, d_recs, d_rat = (torch.from_numpy(a).cuda() for a in (tab, wf, recs, rat))

    def call(t=tab, f=wf, r=recs, q=rat, rows=d_rows, n_rows=W, stride=stride, nwin=W, nrec=3, core=CORE, context=CONTEXT, out=out,
             dev=d_tab):
        t, f, r, q = (np.ascontiguousarray(a) for a in (t, f, r, q))
        return _raw(L.ptr(rows), n_rows, stride, L.ptr(dev), t.ctypes.data, L.ptr(d_wf), f.ctypes.data, nwin, L.ptr(d_recs),
                    r.ctypes.data, L.ptr(d_rat), q.ctypes.data, nrec, core, context, L.ptr(out))

    def changed(a, i, col, value):
        a = a.copy()
        if a.ndim == 1:
            a[i] = value
        else:
            a[i, col] = value
        return a

    assert call()[0] == 0
    for kw in (dict(rows=None), dict(out=None), dict(dev=None)):
        rc, msg = call(**kw)
        assert rc == -22 and "null pointer" in msg, msg
    for kw in (dict(nwin=0), dict(nwin=65536), dict(stride=0), dict(nrec=0), dict(nrec=65536), dict(core=0), dict(context=-1),
               dict(core=2 * CONTEXT - 1), dict(n_rows=0)):
        rc, msg = call(**kw)
        assert rc == -22 and "bad args" in msg, (kw, msg)
    for what, kw, name in (("a row outside the rows", dict(t=changed(tab, 2, 7, W)), "window 2 "),
                           ("a negative row", dict(t=changed(tab, 1, 7, -1)), "window 1 "),
                           ("fewer rows than the table names", dict(n_rows=W - 1), "window %d " % (W - 1)),
                           ("more frames than the stride", dict(f=changed(wf, 3, 0, stride + 1)), "window 3 "),
                           ("no frames", dict(f=changed(wf, 0, 0, 0)), "window 0 "),
                           ("a negative start", dict(t=changed(tab, 4, 6, -1)), "window 4 "),
                           ("windows outside the table", dict(r=changed(recs, 2, 2, W - 1)), "recording 2 "),
                           ("no windows", dict(r=changed(recs, 1, 3, 0)), "recording 1 "),
                           ("frames past the summed output", dict(r=changed(recs, 2, 0, recs[2, 0] + 1)), "recording 2 "),
                           ("a negative frame count", dict(r=changed(recs, 0, 1, -1)), "recording 0 "),
                           ("a ratio of zero", dict(q=changed(rat, 1, 0, 0.0)), "recording 1 "),
                           ("a ratio that is no number", dict(q=changed(rat, 2, 0, np.nan)), "recording 2 ")):
        rc, msg = call(**kw)
        assert rc == -22 and msg.startswith("sos_window_frames_stitch_f32: ") and name in msg, (what, msg)


def _spared(a, fill=0):
    a = np.asarray(a).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.full(SPARE, fill, a.dtype)])).cuda()


def test_kernel_skips_a_device_entry_that_leaves_the_hosts_sizes():
    """The device rule: the host tables are correct, a DEVICE table differs in one entry.  The call succeeds, the frames that
    need the entry are left as they were, everything else is what the unaltered call gives, nothing past the buffers is
    written (spare elements behind every buffer keep a wrongly followed entry inside allocated memory)."""
    from sos_amd import _lib as L
    fps = 25.0
    tab, wf, rows, recs, refs = _case(NS[:3], fps)
    rat = np.full(3, SR / fps)
    W, stride, total = len(tab), rows.shape[1], int(recs[:, 1].sum())
    d_rows = _spared(rows)

    def run(t=tab, f=wf, r=recs, q=rat):
        out = torch.full((total + SPARE,), SENTINEL, device="cuda")
        d = [_spared(a) for a in (t, f, r, q)]
        rc = L.lib().sos_window_frames_stitch_f32(L.ptr(d_rows), W, stride, L.ptr(d[0]), tab.ctypes.data, L.ptr(d[1]), wf.ctypes.data,
                                                  W, L.ptr(d[2]), recs.ctypes.data, L.ptr(d[3]), rat.ctypes.data, 3, CORE, CONTEXT,
                                                  L.ptr(out), L.stream_ptr())
        assert rc == 0
        return out.cpu().numpy()

    def changed(a, i, col, value):
        a = a.copy()
        if a.ndim == 1:
            a[i] = value
        else:
            a[i, col] = value
        return a

    base = run()
    assert not (base[:total] == SENTINEL).any() and (base[total:] == SENTINEL).all()
    # a recording's entry: all of its frames are skipped
    for r, col, value in ((1, 0, total), (1, 1, recs[1, 1] + recs[2, 1] + 1), (2, 2, W - 1), (0, 3, W + 1), (1, 3, 0), (2, 0, -1)):
        got = run(r=changed(recs, r, col, value))
        lo, hi = int(recs[r, 0]), int(recs[r, 0] + recs[r, 1])
        assert (got[lo:hi] == SENTINEL).all() and (got[total:] == SENTINEL).all(), (r, col, value)
        assert _same_bits(got[:lo], base[:lo]) and _same_bits(got[hi:total], base[hi:total]), (r, col, value)
    got = run(q=changed(rat, 1, 0, -1.0))
    lo, hi = int(recs[1, 0]), int(recs[1, 0] + recs[1, 1])
    assert (got[lo:hi] == SENTINEL).all() and _same_bits(got[:lo], base[:lo]) and _same_bits(got[hi:total], base[hi:total])
    # a window's entry (window 2 = the middle one of recording 1): the frames it owns and the neighbours' frames that blend
    # with it are skipped, every other frame is untouched
    st = refs[1]
    needs = (st.owner == 1) | (st.other == 1)
    lo = int(recs[1, 0])
    for what, kw in (("row", dict(t=changed(tab, 2, 7, W))), ("row", dict(t=changed(tab, 2, 7, -1))),
                     ("frames", dict(f=changed(wf, 2, 0, stride + 1))), ("frames", dict(f=changed(wf, 2, 0, 0)))):
        got = run(**kw)
        mine = got[lo:lo + len(needs)]
        assert (mine[needs] == SENTINEL).all() and _same_bits(mine[~needs], base[lo:lo + len(needs)][~needs]), what
        assert _same_bits(got[:lo], base[:lo]) and _same_bits(got[lo + len(needs):total], base[lo + len(needs):total])
        assert (got[total:] == SENTINEL).all()
