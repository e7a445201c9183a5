"""The host-side validation of sos_window_stitch_planes_f32 (csrc/ragged_window.hip) returns before any launch, so it runs
without a device: the pointers are dummies that are never followed (as in test_window_reference.py).  Every refusal is -22
(SOS_EINVAL) and names the window or the recording."""
import ctypes as C

import numpy as np

import window_reference as R

NS = [31, 5, 100]                   # 3 windows, 1 window, 12 windows at core 8 / context 4 and hop 1
STRIDE = 24


def _case():
    tab = R.table(R.plan(NS, 8, 4, hop=1, min_frames=1), NS, hop=1)
    total = sum(NS)
    recs = np.ascontiguousarray(np.stack([np.cumsum(NS) - NS, np.full(len(NS), total)], axis=1).astype(np.int64))
    return tab, recs, total


def _call(h, P, tab, recs, *, planes=4, n_rows=None, stride=STRIDE, nwin=None, context=4, nrec=None, out_total=None, rows=None,
          out=None, dev=None, dev_recs=None, host=True, host_recs=True):
    tab, recs = np.ascontiguousarray(tab), np.ascontiguousarray(recs)
    total = sum(NS)
    rc = h.sos_window_stitch_planes_f32(P if rows is None else rows, planes, len(tab) if n_rows is None else n_rows, stride,
                                        P if dev is None else dev, tab.ctypes.data if host else None,
                                        len(tab) if nwin is None else nwin, context, P if dev_recs is None else dev_recs,
                                        recs.ctypes.data if host_recs else None, len(recs) if nrec is None else nrec,
                                        planes * total if out_total is None else out_total, P if out is None else out, None)
    return rc, h.sos_last_error().decode()


def test_the_planes_stitch_refuses_on_the_host_and_names_the_window_or_the_recording():
    from sos_amd import _lib as L
    h = L.lib()
    tab, recs, total = _case()
    W = len(tab)
    assert W == 16
    P, NULL = C.c_void_p(1 << 20), C.c_void_p(0)

    def changed(a, i, col, value):
        a = a.copy()
        a[i, col] = value
        return a

    def call(t=tab, r=recs, **kw):
        return _call(h, P, t, r, **kw)

    file_major = np.asarray([[0, 32], [4 * 32, 8], [4 * 40, 100]], dtype=np.int64)            # pitches 31 + 1, 5 + 3, 100 + 0
    shifted = tab.copy()                                # the one window of recording 1 with its core a sample later: the same sum
    shifted[3, 2], shifted[3, 4], shifted[3, 5] = 6, 1, 6
    cases = [
        # arguments
        (call(rows=NULL), "null pointer"), (call(out=NULL), "null pointer"), (call(dev=NULL), "null pointer"),
        (call(dev_recs=NULL), "null pointer"), (call(host=False), "null pointer"), (call(host_recs=False), "null pointer"),
        (call(planes=0), "1 .. 8 planes, got 0"), (call(planes=9), "1 .. 8 planes, got 9"), (call(planes=-1), "planes, got -1"),
        (call(nrec=0), "recordings, got 0"), (call(nrec=65536), "recordings, got 65536"),
        (call(out_total=-1), "an output of -1 floats"),
        # everything sos_window_stitch_f32 refuses, column 3 included
        (call(nwin=0), "bad args"), (call(nwin=65536), "bad args"), (call(stride=0), "bad args"), (call(context=-1), "context -1"),
        (call(context=(1 << 22) + 1), "bad args"),
        (call(t=changed(tab, 2, 2, STRIDE + 1)), "window 2 has more samples than the stride"),
        (call(t=changed(tab, 4, 7, W)), "window 4 names a row outside"),
        (call(n_rows=W - 1), "window 15 names a row outside"),
        (call(t=changed(tab, 15, 3, tab[15, 3] + 1)), "window 15 writes outside the summed output length"),
        (call(t=changed(tab, 1, 6, tab[1, 4] + 1)), "window 1 has a core outside"),
        (call(t=changed(tab, 1, 9, W)), "window 1 names a neighbour"),
        (call(t=changed(tab, 1, 9, 15)), "window 1 names a neighbour"),
        (call(context=12), "window 0 blends over a context that is not less than the window"),
        (call(context=5), "window 0 "),
        (call(t=changed(tab, 3, 5, -1)), "window 3 has the core"),
        # the recordings
        (call(t=changed(tab, 3, 0, 3)), "window 3 names recording 3 of 3"),
        (call(t=changed(tab, 3, 0, -1)), "window 3 names recording -1 of 3"),
        (call(nrec=2), "window 4 names recording 2 of 2"),
        (call(t=changed(tab, 1, 0, 1)), "window 0 of recording 0 has the neighbour 1, a window of recording 1"),
        (call(t=shifted), "window 3 has the core 1 .. 6, outside the 5 output samples of recording 1"),
        (call(r=changed(recs, 2, 1, 99)), "recording 2 has the pitch 99, less than its 100 output samples"),
        (call(r=changed(recs, 0, 1, -1)), "recording 0 has the pitch -1"),
        (call(r=changed(recs, 1, 0, -1)), "recording 1 (base -1"),
        (call(r=changed(recs, 2, 0, 37)), "recording 2 (base 37, pitch 136, 100 samples in each of 4 planes) lies outside the 544"),
        (call(out_total=4 * total - 1), "recording 2 "),
        (call(r=changed(recs, 2, 1, 1 << 62)), "recording 2 "),
        (call(r=changed(recs, 1, 0, 30)), "plane 0 of recording 0 (0 + 31) and plane 0 of recording 1 (from 30) overlap"),
        (call(r=changed(recs, 1, 0, 131)), "plane 0 of recording 2 (36 + 100) and plane 0 of recording 1 (from 131) overlap"),
        (call(r=changed(file_major, 1, 0, 4 * 32 - 2), out_total=4 * 140),
         "plane 3 of recording 0 (96 + 31) and plane 0 of recording 1 (from 126) overlap"),
        (call(r=changed(file_major, 0, 1, 30), out_total=4 * 140), "recording 0 has the pitch 30"),
        (call(r=file_major, out_total=4 * 140 - 1), "recording 2 "),
    ]
    for (rc, msg), want in cases:
        assert rc == -22 and want in msg and msg.startswith("sos_window_stitch_planes_f32: "), (want, rc, msg)


def test_the_abi_version_is_unchanged():
    from sos_amd import _lib as L
    assert L.lib().sos_abi_version() == 10 and "sos_window_stitch_planes_f32" in L.SIGNATURES
