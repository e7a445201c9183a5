"""The host half of sos_window_frames_link_f32 (csrc/ragged_window.hip) and of the layers above it: what they answer to tables
and arguments with one defect.  Every call is refused on the host before anything is launched -- the pointers to device memory
are dummies that are never dereferenced and the waveforms are CPU tensors, so no GPU is needed
(tests/test_window_decisions_host_cpu.py checks the neighbouring entry points the same way).  Also: the package's link-table
helper against tests/link_reference.py's, and that reference's own properties."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import frames_reference as FR
import link_reference as LR
import window_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_buf = (C.c_float * 64)()
P = C.cast(_buf, C.c_void_p)                     # stands for every device pointer
HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
N_ONE, N_LONG = 150 * HOP + 31, 3 * CORE + 5 * HOP + 77
NS = [N_ONE, N_LONG, N_ONE, N_LONG]              # recordings 1 and 3 are linked, 0 and 2 stand alone
IDS = [None, "pair", None, "pair"]
SR, FPS = 14000, 30.0
SECONDS = dict(window_seconds=CORE / SR, context_seconds=CONTEXT / SR)
NAME = "sos_window_frames_link_f32"


def _host(a):
    return a.ctypes.data_as(C.c_void_p)


def _tables():
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
    links, members, _ = LR.tables(IDS, recs[:, 1])
    return dict(tab=tab, wf=np.asarray(wf, dtype=np.int64), recs=recs, rat=np.full(len(NS), SR / FPS), links=links, members=members)


def _link(n_rows=8, stride=60, nwin=8, nrec=4, core=CORE, context=CONTEXT, ngroups=3, mode=0, threshold=0.5, rows=P, out_logits=P,
          out_bits=P, links_dev=P, members_dev=P, **tables):
    from sos_amd import _lib as L
    t = {k: np.ascontiguousarray(tables.get(k, v)) for k, v in _tables().items()}
    rc = L.lib().sos_window_frames_link_f32(rows, n_rows, stride, P, _host(t["tab"]), P, _host(t["wf"]), nwin, P, _host(t["recs"]), P,
                                            _host(t["rat"]), nrec, core, context, links_dev, _host(t["links"]), members_dev,
                                            _host(t["members"]), ngroups, mode, threshold, out_logits, out_bits, None)
    return rc, L.lib().sos_last_error().decode()


def _set(a, i, col, value):
    a = a.copy()
    if a.ndim == 1:
        a[i] = value
    else:
        a[i, col] = value
    return a


def test_the_tables_are_one_pair_between_two_single_recordings():
    t = _tables()
    assert t["tab"].shape == (8, 10) and list(t["recs"][:, 3]) == [1, 3, 1, 3] and t["wf"].max() <= 60
    assert t["links"].tolist() == [[0, 51, 0, 1], [51, 83, 1, 2], [134, 51, 3, 1]] and t["members"].tolist() == [0, 1, 3, 2]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_the_symbol_is_declared_bound_and_exported_by_both_libraries(precision):
    import sos_amd
    from sos_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sos_hip.h")).read()
    assert re.search(r"\bint %s\s*\(" % NAME, hdr)
    assert len(L.SIGNATURES[NAME]) == 25 and len(L.SIGNATURES["sos_window_frames_stitch_f32"]) == 17
    sos_amd.set_precision(precision)
    try:
        h = L.lib()
    finally:
        sos_amd.set_precision("bf16")
    assert hasattr(h, NAME) and h.sos_abi_version() == L.EXPECTED_ABI == 10


@pytest.mark.parametrize("kw,fragments", [
    (dict(rows=None), ["null pointer"]),
    (dict(out_logits=None), ["null pointer"]),
    (dict(out_bits=None), ["null pointer"]),
    (dict(links_dev=None), ["null pointer"]),
    (dict(members_dev=None), ["null pointer"]),
    (dict(ngroups=0), ["bad args", "1 .. 65535 groups, got 0"]),
    (dict(ngroups=65536), ["bad args", "got 65536"]),
    (dict(mode=2), ["bad args", "mode 2"]),
    (dict(mode=-1), ["bad args", "mode -1"]),
    (dict(threshold=float("nan")), ["bad args", "threshold nan"]),
    (dict(threshold=float("inf")), ["bad args", "threshold inf"]),
    (dict(links=(1, 3, 0)), ["group 1 has no members"]),
    (dict(links=(1, 3, 5)), ["group 1 has a member count of 5"]),
    (dict(links=(2, 2, 4)), ["group 2 ", "members 4 + 1 of 4"]),
    (dict(members=(1, 0, 4)), ["member 0 of group 1 names recording 4 of 4"]),
    (dict(members=(2, 0, -1)), ["member 1 of group 1 names recording -1 of 4"]),
    (dict(members=(3, 0, 0)), ["recording 0 appears twice", "member 0 of group 2 and in group 0"]),
    (dict(members=(2, 0, 1)), ["recording 1 appears twice", "member 1 of group 1 and in group 1"]),
    (dict(recs=(3, 1, 82)), ["recording 3, member 1 of group 1, has 82 frames", "its group has 83 frames"]),
    (dict(links=(2, 1, 50)), ["recording 2, member 0 of group 2, has 51 frames", "its group has 50 frames"]),
    (dict(rat=(3, 0, SR / 25.0)), ["recording 3, member 1 of group 1", "560 samples", "share one frame grid"]),
    (dict(links=(2, 0, 135)), ["group 2 (frames 135 + 51 of 185", "lies outside the summed output"]),
    (dict(links=(2, 0, 100)), ["group 1 and group 2 overlap in the output"]),
    (dict(links=(0, 1, -1)), ["group 0 has -1 frames"]),
    # every check of sos_window_frames_stitch_f32 on the recordings and windows that are members
    (dict(nwin=0), ["bad args", "got 0"]),
    (dict(nrec=65536), ["bad args", "got 65536"]),
    (dict(stride=0), ["bad args"]),
    (dict(core=0), ["bad args", "core 0"]),
    (dict(context=-1), ["bad args", "context -1"]),
    (dict(core=2 * CONTEXT - 1), ["bad args", "twice the context"]),
    (dict(tab=(2, 7, 8)), ["window 2 of recording 1", "row 8 of 8"]),
    (dict(tab=(5, 7, -1)), ["window 5 of recording 3", "row -1 of 8"]),
    (dict(n_rows=7), ["window 7 of recording 3", "row 7 of 7"]),
    (dict(wf=(6, 0, 61)), ["window 6 of recording 3", "frames 61, stride 60"]),
    (dict(wf=(0, 0, 0)), ["window 0 of recording 0", "frames 0"]),
    (dict(tab=(4, 6, -1)), ["window 4 of recording 2", "start -1"]),
    (dict(recs=(3, 2, 6)), ["recording 3, member 1 of group 1", "windows 6 + 3 of 8"]),
    (dict(recs=(0, 3, 0)), ["recording 0, member 0 of group 0", "windows 0 + 0 of 8"]),
    (dict(rat=(2, 0, 0.0)), ["recording 2, member 0 of group 2", "0 samples per frame"]),
    (dict(rat=(0, 0, float("nan"))), ["recording 0, member 0 of group 0", "nan samples per frame"]),
])
def test_link_refuses_one_defect_by_name(kw, fragments):
    base = _tables()
    kw = {k: _set(base[k], *v) if k in base else v for k, v in kw.items()}
    rc, msg = _link(**kw)
    assert rc == -22 and msg.startswith(NAME + ": "), (rc, msg)
    for f in fragments:
        assert f in msg, (f, msg)


def test_a_recording_in_no_group_is_not_read():
    """Two groups only: recording 2 (the last member listed) belongs to none, and its defects do not matter.  The call gets past
    the host checks only with real device memory, so what is shown here is that the refusal names another, later defect."""
    base = _tables()
    links, members = base["links"][:2].copy(), base["members"][:3].copy()
    recs = _set(_set(base["recs"], 2, 3, 0), 2, 1, -5)                    # recording 2: no windows, a negative frame count
    rc, msg = _link(links=links, members=members, recs=recs, ngroups=2, tab=_set(base["tab"], 7, 7, 99))
    assert rc == -22 and "window 7 of recording 3" in msg, msg


@pytest.mark.parametrize("ids", [
    [0, 1, 0, 1, 2, 0],                         # interleaved
    [None, "a", None, "a", None],               # None entries between the members of a group
    [None, None, None],                         # groups of one
    [5, 6, 7],
    [3, 3, 3, 3],
    ["L", None, "R", "L", None, "R"],
])
def test_the_packages_link_tables_equal_the_references(ids):
    from sos_amd import tools
    frames = [40 + 3 * (r if g is None else ids.index(g)) for r, g in enumerate(ids)]         # equal within a group
    want, got = LR.tables(ids, frames), tools.link_tables(ids, frames)
    for w, g in zip(want, got):
        assert g.dtype == np.int64 and w.shape == g.shape and np.array_equal(w, g)
    links, members, group = got
    assert sorted(members.tolist()) == list(range(len(ids))) and links[:, 3].sum() == len(ids)
    assert np.array_equal(links[:, 0], np.cumsum(links[:, 1]) - links[:, 1])
    firsts = [int(members[f]) for f in links[:, 2]]
    assert firsts == sorted(firsts)                                       # groups in first-appearance order
    for r, g in enumerate(group):
        assert r in members[links[g, 2]:links[g, 2] + links[g, 3]]


def _clips(ns):
    return [torch.zeros(n) for n in ns]


def test_detect_long_refuses_bad_links_without_a_device():
    from sos_amd import pipeline, windows
    assert pipeline.detect_long is windows.detect_long
    with pytest.raises(ValueError, match="link must hold one group id"):
        windows.detect_long(None, _clips([N_ONE, N_ONE]), link=[0], **SECONDS)
    with pytest.raises(ValueError, match="link_mode"):
        windows.detect_long(None, _clips([N_ONE, N_ONE]), link=[0, 0], link_mode="max", **SECONDS)
    with pytest.raises(ValueError, match="link_mode"):
        windows.detect_long(None, _clips([N_ONE]), link_mode="median", **SECONDS)
    with pytest.raises(ValueError, match="recording 1 has %d samples" % (N_ONE + 1)):
        windows.detect_long(None, _clips([N_ONE, N_ONE + 1]), link=[0, 0], **SECONDS)
    with pytest.raises(ValueError, match="recording 2 has .* 25.0 fps"):
        windows.detect_long(None, _clips([N_ONE, N_ONE, N_ONE]), fps=[30.0, 30.0, 25.0], link=["a", None, "a"], **SECONDS)
    with pytest.raises(ValueError, match="recording 1 has .* and 50 frames"):
        windows.detect_long(None, _clips([N_ONE, N_ONE]), n_frames=[51, 50], link=[7, 7], **SECONDS)


def test_denoise_long_refuses_a_link_without_stitch_bits_without_a_device():
    from sos_amd import windows
    with pytest.raises(ValueError, match="stitch_bits=True"):
        windows.denoise_long(None, None, _clips([N_ONE, N_ONE]), link=[0, 0], **SECONDS)
    with pytest.raises(ValueError, match="stitch_bits=True"):
        windows.denoise_long(None, None, _clips([N_ONE, N_ONE]), link=[0, 0], bits=[np.zeros(51, np.uint8)] * 2, **SECONDS)
    with pytest.raises(ValueError, match="link must hold one group id"):
        windows.denoise_long(None, None, _clips([N_ONE, N_ONE]), stitch_bits=True, link=[0, 0, 0], **SECONDS)
    with pytest.raises(ValueError, match="link_mode"):
        windows.denoise_long(None, None, _clips([N_ONE, N_ONE]), stitch_bits=True, link=[0, 0], link_mode="all", **SECONDS)
    with pytest.raises(ValueError, match="recording 1 has %d samples" % N_LONG):
        windows.denoise_long(None, None, _clips([N_ONE, N_LONG]), stitch_bits=True, link=[0, 0], **SECONDS)


def test_denoise_recordings_refuses_an_unknown_link_channels_before_it_reads_a_file(tmp_path):
    from sos_amd import recordings
    out_dir = tmp_path / "out"
    for bad in ("max", "ANY", True, 0):
        with pytest.raises(ValueError, match="link_channels"):
            recordings.denoise_recordings(None, None, [str(tmp_path / "missing.wav")], str(out_dir), link_channels=bad)
    assert not out_dir.exists()


def test_window_frames_link_checks_its_arguments_like_window_frames_stitch():
    from sos_amd import tools
    t = _tables()
    with pytest.raises((ValueError, RuntimeError)):                      # CPU rows: there is no fall-back
        tools.window_frames_link(torch.zeros(8, 60), t["tab"], t["wf"], t["recs"], SR / FPS, CORE, CONTEXT, t["links"], t["members"], "any")
    assert tools.LINK_MODES == {"any": 0, "mean": 1}


def test_reference_a_group_of_one_is_its_member_bit_for_bit():
    x = np.random.default_rng(5).standard_normal(1000).astype(np.float32)
    x[:4] = [0.0, -0.0, 1e-7, -1e-7]
    x[4] = np.float32(1e-45)                                              # a denormal survives the divide by one
    for mode in LR.MODES:
        assert np.array_equal(LR.link([x], mode).view(np.uint32), x.view(np.uint32)), mode


def test_reference_any_is_invariant_under_member_order_and_mean_is_the_f32_sum():
    rng = np.random.default_rng(6)
    rows = [rng.standard_normal(500).astype(np.float32) for _ in range(3)]
    want = LR.link(rows, "any")
    for order in ([1, 0, 2], [2, 1, 0], [1, 2, 0]):
        assert np.array_equal(LR.link([rows[k] for k in order], "any").view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want, np.max(rows, axis=0))
    mean = LR.link(rows, "mean")
    assert mean.dtype == np.float32 and np.array_equal(mean, ((rows[0] + rows[1]) + rows[2]) / np.float32(3))
    assert np.abs(mean - np.mean(np.asarray(rows, np.float64), axis=0)).max() < 1e-6


def test_reference_decides_zero_as_speech_at_one_half():
    assert LR.decide(0.0, 0.5) == 1 and LR.decide(np.float32(1e-7), 0.5) == 1
    x = np.asarray([-100.0, -1.0, 0.0, 1.0, 100.0], np.float32)
    assert LR.decide(x, 0.5).tolist() == [0, 0, 1, 1, 1] and LR.decide(x, 0.5).dtype == np.uint8
    assert LR.decide(x, 0.75).tolist() == [0, 0, 0, 0, 1]
    assert LR.near_threshold(np.asarray([0.0, 1e-7, -1e-7, 1e-5, -1e-5, 0.3], np.float32)).tolist() == [True, True, True, False, False, False]
