"""Pins tests/window_reference.py, the float64 restatement of the windowing of long recordings (CPU only): hand-worked plans, the
refusals, that the cores tile every output and every sample is covered by one or two windows, that the weights of an overlap
sum to 1 -- and that sos_amd.pipeline.window_plan, which the launch sequence follows, is the same plan."""
import numpy as np
import pytest

import window_reference as R
from window_reference import Window

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP                        # 12640 and 1264 samples


def test_the_hop_and_the_shortest_clip_are_the_packages():
    from sos_amd import pipeline, transform
    assert R.HOP == transform.HOP_LENGTH == HOP and R.MIN_FRAMES == pipeline.MIN_FRAMES


@pytest.mark.parametrize("n,want", [
    # one sample short of two cores: n_out = 159 hops = 25122 < 2 core, one window, the whole recording
    (2 * CORE - 1, [Window(0, 0, 25279, 0, 25122)]),
    # two cores: the first window reads a context past its core, the second a context before it; both the minimum length
    (2 * CORE, [Window(0, 0, 13904, 0, 12640), Window(0, 11376, 13904, 12640, 25280)]),
    # 3 core + hop + 7: the last core takes the extra hop, the last window the 7 samples of the tail too
    (3 * CORE + HOP + 7, [Window(0, 0, 13904, 0, 12640), Window(0, 11376, 15168, 12640, 25280),
                          Window(0, 24016, 14069, 25280, 38078)]),
    # the shortest recording the plan's arguments promise to handle as a window
    (CORE + CONTEXT, [Window(0, 0, 13904, 0, 13904)]),
], ids=["2core-1", "2core", "3core+hop+7", "core+context"])
def test_hand_worked_plans(n, want):
    assert R.plan([n], CORE, CONTEXT) == want
    # core and context are rounded up to whole hops
    assert R.plan([n], CORE - HOP + 1, CONTEXT - 1) == want


def test_refusals():
    with pytest.raises(ValueError):
        R.plan([10 * CORE], CORE, CORE // 2 + HOP)           # core < 2 context
    with pytest.raises(ValueError):
        R.plan([10 * CORE], 60 * HOP, 4 * HOP)               # a window of 64 hops
    assert len(R.plan([10 * CORE], 60 * HOP, 5 * HOP)) == 10 * 80 // 60
    with pytest.raises(ValueError, match="recording 1"):
        R.plan([CORE, 64 * HOP - 1, CORE], CORE, CONTEXT)    # 64 frames
    assert len(R.plan([64 * HOP], CORE, CONTEXT)) == 1       # 65 frames


LENGTHS = [64 * HOP, 64 * HOP + 157, CORE + CONTEXT, 2 * CORE - 1, 2 * CORE, 2 * CORE + 1, 3 * CORE + HOP + 7, 7 * CORE + 3 * HOP,
           10 * CORE - 1, 23 * CORE + 11]


@pytest.mark.parametrize("core,context", [(CORE, CONTEXT), (CORE, 0), (CORE, CORE // 2), (65 * HOP, 0), (130 * HOP, 65 * HOP)])
def test_cores_tile_the_output_and_windows_cover_it_once_or_twice(core, context):
    wins = R.plan(LENGTHS, core, context)
    assert [w.recording for w in wins] == sorted(w.recording for w in wins)
    for r, n in enumerate(LENGTHS):
        mine = [w for w in wins if w.recording == r]
        n_out = HOP * (n // HOP)
        assert len(mine) == max(1, n_out // core)
        assert mine[0].core_start == 0 and mine[-1].core_end == n_out
        assert all(a.core_end == b.core_start for a, b in zip(mine, mine[1:]))
        assert all(core <= w.core_end - w.core_start < 2 * core for w in mine) or len(mine) == 1
        cover = np.zeros(n_out, dtype=np.int64)
        for k, w in enumerate(mine):
            assert w.start % HOP == 0 and (w.samples % HOP == 0 or k == len(mine) - 1)
            assert 1 + w.samples // HOP >= R.MIN_FRAMES
            assert w.start + w.samples <= n and (k < len(mine) - 1 or w.start + w.samples == n)
            row_end = w.start + HOP * (w.samples // HOP)                    # what the window's denoised row covers
            assert w.start <= max(w.core_start - context, 0) and min(w.core_end + context, n_out) <= row_end
            cover[w.start:row_end] += 1
        assert cover.min() >= 1 and cover.max() <= 2
        # covered twice: exactly the overlap zones
        twice = np.zeros(n_out, dtype=bool)
        for w in mine[:-1]:
            twice[w.core_end - context:w.core_end + context] = True
        assert np.array_equal(cover == 2, twice)


@pytest.mark.parametrize("context", [1, 4, 158, 1264, 28124])
def test_weights_of_an_overlap_sum_to_one(context):
    w = R.weights(context)
    assert len(w) == 2 * context and 0 < w[0] < w[-1] < 1
    assert np.allclose(w + w[::-1], 1.0, rtol=0, atol=2e-16)               # the two windows swap roles under reflection
    assert np.array_equal((1.0 - w) + w, np.ones(2 * context))
    # stitching a signal with itself returns it
    x = np.random.default_rng(context).standard_normal(4 * context + 5)
    wins = [Window(0, 0, 3 * context, 0, 2 * context), Window(0, context, 3 * context + 5, 2 * context, 4 * context + 5)]
    out, blended = R.stitch(wins, [x[:3 * context], x[context:]], context)
    assert np.allclose(out, x, rtol=0, atol=1e-15) and blended.sum() == 2 * context
    assert np.array_equal(out[~blended], x[~blended])


@pytest.mark.parametrize("core,context", [(CORE, CONTEXT), (CORE - 3, CONTEXT - 157), (CORE, 0), (65 * HOP, 0), (30 * 14000, 2 * 14000)])
def test_window_plan_of_the_package_is_the_restatement(core, context):
    from sos_amd import pipeline
    got = pipeline.window_plan(LENGTHS, core, context)
    want = R.table(R.plan(LENGTHS, core, context), LENGTHS)
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)


def test_window_plan_of_the_package_refuses_what_the_restatement_refuses():
    from sos_amd import pipeline
    for ns, core, context in (([10 * CORE], CORE, CORE // 2 + HOP), ([10 * CORE], 60 * HOP, 4 * HOP), ([CORE, 64 * HOP - 1], CORE, CONTEXT)):
        with pytest.raises(ValueError):
            R.plan(ns, core, context)
        with pytest.raises(ValueError):
            pipeline.window_plan(ns, core, context)
    with pytest.raises(ValueError, match="recording 1"):
        pipeline.window_plan([CORE, 64 * HOP - 1], CORE, CONTEXT)


def test_the_two_entry_points_refuse_on_the_host_and_name_the_window():
    """The host-side validation of sos_window_stage_f32 / sos_window_stitch_f32 returns before any launch, so it runs without a
    device: the pointers are dummies that are never followed."""
    import ctypes as C
    from sos_amd import _lib as L
    h = L.lib()
    ns = [31, 5, 100]
    tab = R.table(R.plan(ns, 8, 4, hop=1, min_frames=1), ns, hop=1)
    W, stride, total = len(tab), 24, sum(ns)
    P = C.c_void_p(1 << 20)

    def stage(t=tab, x=P, total=total, nwin=W, stride=stride):
        t = np.ascontiguousarray(t)
        return h.sos_window_stage_f32(x, total, P, t.ctypes.data, nwin, stride, P, None), h.sos_last_error().decode()

    def stitch(t=tab, n_rows=W, stride=stride, nwin=W, context=4, out=P):
        t = np.ascontiguousarray(t)
        return h.sos_window_stitch_f32(P, n_rows, stride, P, t.ctypes.data, nwin, context, out, None), h.sos_last_error().decode()

    def changed(w, col, value):
        t = tab.copy()
        t[w, col] = value
        return t

    for (rc, msg), want in ((stage(x=None), "null pointer"), (stitch(out=None), "null pointer"),
                            (stage(nwin=0), "bad args"), (stage(nwin=65536), "bad args"), (stage(stride=0), "bad args"),
                            (stitch(nwin=0), "bad args"), (stitch(nwin=65536), "bad args"), (stitch(stride=0), "bad args"),
                            (stitch(context=-1), "context -1"),
                            (stage(t=changed(2, 2, stride + 1)), "window 2 has 25 samples"),
                            (stitch(t=changed(2, 2, stride + 1)), "window 2 has more samples than the stride"),
                            (stage(t=changed(3, 1, total - 4)), "window 3 (samples 132 + 5) lies outside the 136"),
                            (stage(t=changed(1, 1, -1)), "window 1 "),
                            (stage(total=total - 1), "window 15 "),
                            (stitch(t=changed(4, 7, W)), "window 4 names a row outside"),
                            (stitch(n_rows=W - 1), "window 15 names a row outside"),
                            (stitch(t=changed(15, 3, tab[15, 3] + 1)), "window 15 writes outside the summed output length"),
                            (stitch(t=changed(1, 6, tab[1, 4] + 1)), "window 1 has a core outside"),
                            (stitch(t=changed(1, 9, W)), "window 1 names a neighbour"),
                            (stitch(t=changed(1, 9, 15)), "window 1 names a neighbour"),
                            (stitch(context=12), "window 0 blends over a context that is not less than the window"),
                            (stitch(context=5), "window 0 ")):
        assert rc == -22 and want in msg, (want, rc, msg)
