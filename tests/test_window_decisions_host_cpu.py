"""The host half of sos_window_frames_stitch_f32 and sos_window_stage_masked_f32 (csrc/ragged_window.hip): what they answer to
tables with one defect.  Every call below is refused on the host before anything is launched -- the pointers to device memory
are dummies that are never dereferenced, so no GPU is needed (tests/test_ragged_host_cpu.py checks the ragged layer the same
way).  The plan is tests/window_reference.py's, the frame counts tests/frames_reference.py's."""
import ctypes as C

import numpy as np
import pytest

import frames_reference as FR
import window_reference as R

_buf = (C.c_float * 64)()
P = C.cast(_buf, C.c_void_p)                     # stands for every device pointer
HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
NS = [150 * HOP + 31, 3 * CORE + 5 * HOP + 77]
SR, FPS = 14000, 30.0


def _host(a):
    return a.ctypes.data_as(C.c_void_p)


def _tables():
    wins = R.plan(NS, CORE, CONTEXT)
    tab = R.table(wins, NS)
    wf = np.asarray(FR.window_frames(wins[:1], SR, FPS) + FR.window_frames(wins[1:], SR, FPS), dtype=np.int64)
    F = [FR.n_video_frames(n, SR, FPS) for n in NS]
    recs = np.asarray([(0, F[0], 0, 1), (F[0], F[1], 1, 3)], dtype=np.int64)
    clips = np.asarray([(0, NS[0], 0, F[0]), (NS[0], NS[1], F[0], F[1])], dtype=np.int64)
    return tab, wf, recs, clips, np.full(2, SR / FPS)


def _frames(tab=None, wf=None, recs=None, rat=None, n_rows=4, stride=60, nwin=4, nrec=2, core=CORE, context=CONTEXT, rows=P):
    from sos_amd import _lib as L
    t, f, r, _, q = _tables()
    t, f, r, q = (np.ascontiguousarray(b if a is None else a) for a, b in ((tab, t), (wf, f), (recs, r), (rat, q)))
    rc = L.lib().sos_window_frames_stitch_f32(rows, n_rows, stride, P, _host(t), P, _host(f), nwin, P, _host(r), P, _host(q), nrec,
                                              core, context, P, None)
    return rc, L.lib().sos_last_error().decode()


def _masked(tab=None, clips=None, rat=None, nrec=2, nwin=4, stride=None, bits=P):
    from sos_amd import _lib as L
    t, _, _, c, q = _tables()
    t, c, q = (np.ascontiguousarray(b if a is None else a) for a, b in ((tab, t), (clips, c), (rat, q)))
    stride = int(t[:, 2].max()) if stride is None else stride
    rc = L.lib().sos_window_stage_masked_f32(P, bits, P, _host(c), P, _host(q), nrec, P, _host(t), nwin, stride, P, P, None)
    return rc, L.lib().sos_last_error().decode()


def _set(a, i, col, value):
    a = a.copy()
    if a.ndim == 1:
        a[i] = value
    else:
        a[i, col] = value
    return a


def test_the_tables_are_the_plan_of_one_and_three_windows():
    tab, wf, recs, clips, rat = _tables()
    assert tab.shape == (4, 10) and list(recs[:, 3]) == [1, 3] and wf.max() <= 60 and recs[:, 1].sum() == 51 + 83
    assert np.array_equal(tab[:, 1], clips[tab[:, 0], 0] + tab[:, 6])              # source offset = the recording's + the start


@pytest.mark.parametrize("kw,fragments", [
    (dict(tab=(2, 7, 4)), ["window 2 of recording 1", "row 4 of 4"]),
    (dict(tab=(1, 7, -1)), ["window 1 of recording 1", "row -1 of 4"]),
    (dict(n_rows=3), ["window 3 of recording 1", "row 3 of 3"]),
    (dict(wf=(3, 0, 61)), ["window 3 of recording 1", "frames 61, stride 60"]),
    (dict(wf=(0, 0, 0)), ["window 0 of recording 0", "frames 0"]),
    (dict(tab=(2, 6, -1)), ["window 2 of recording 1", "start -1"]),
    (dict(recs=(1, 2, 2)), ["recording 1 ", "windows 2 + 3 of 4"]),
    (dict(recs=(0, 3, 0)), ["recording 0 ", "windows 0 + 0 of 4"]),
    (dict(recs=(1, 0, 52)), ["recording 1 ", "frames 52 + 83 of 134"]),
    (dict(recs=(0, 1, -1)), ["recording 0 has -1 frames"]),
    (dict(rat=(1, 0, 0.0)), ["recording 1 ", "0 samples per frame"]),
    (dict(rat=(0, 0, float("nan"))), ["recording 0 ", "nan samples per frame"]),
    (dict(nwin=0), ["bad args", "got 0"]),
    (dict(nwin=65536), ["bad args", "got 65536"]),
    (dict(nrec=0), ["bad args", "1 .. 65535 recordings, got 0"]),
    (dict(nrec=65536), ["bad args", "got 65536"]),
    (dict(stride=0), ["bad args"]),
    (dict(core=0), ["bad args", "core 0"]),
    (dict(context=-1), ["bad args", "context -1"]),
    (dict(core=2 * CONTEXT - 1), ["bad args", "twice the context"]),
    (dict(rows=None), ["null pointer"]),
])
def test_frames_stitch_refuses_one_defect_by_name(kw, fragments):
    base = dict(zip(("tab", "wf", "recs", "_", "rat"), _tables()))
    kw = {k: _set(base[k], *v) if k in base else v for k, v in kw.items()}
    rc, msg = _frames(**kw)
    assert rc == -22 and msg.startswith("sos_window_frames_stitch_f32: "), (rc, msg)
    for f in fragments:
        assert f in msg, (f, msg)


@pytest.mark.parametrize("kw,fragments", [
    (dict(stride=NS[0] - 1), ["window 0 has %d samples (stride %d)" % (NS[0], NS[0] - 1)]),
    (dict(tab=(2, 0, 2)), ["window 2 (recording 2 of 2"]),
    (dict(tab=(0, 0, -1)), ["window 0 (recording -1 of 2"]),
    (dict(tab=(3, 2, 1 << 20), stride=1 << 20), ["window 3 ", "lies outside its recording"]),
    (dict(tab=(1, 1, NS[0] + 1)), ["window 1 ", "its source offset is not its start"]),
    (dict(tab=(0, 2, -1)), ["window 0 ", "samples -1"]),
    (dict(clips=(1, 0, NS[0] + 1)), ["recording 1 (samples %d + %d" % (NS[0] + 1, NS[1]), "lies outside"]),
    (dict(clips=(1, 2, 52)), ["recording 1 ", "frames 52 + 83", "lies outside"]),
    (dict(clips=(0, 1, -1)), ["recording 0 has -1 samples"]),
    (dict(clips=(1, 3, -1)), ["recording 1 has", "-1 frames"]),
    (dict(rat=(1, 0, 1.0)), ["recording 1 has ratio 1 "]),
    (dict(nwin=0), ["bad args"]),
    (dict(nrec=65536), ["bad args", "1 .. 65535 recordings, got 65536"]),
    (dict(bits=None), ["null pointer"]),
])
def test_stage_masked_refuses_one_defect_by_name(kw, fragments):
    base = dict(zip(("tab", "_", "__", "clips", "rat"), _tables()))
    kw = {k: _set(base[k], *v) if k in base else v for k, v in kw.items()}
    rc, msg = _masked(**kw)
    assert rc == -22 and msg.startswith("sos_window_stage_masked_f32: "), (rc, msg)
    for f in fragments:
        assert f in msg, (f, msg)
