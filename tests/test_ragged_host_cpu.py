"""The host half of the ragged layer (csrc/ragged.h, ragged.py): what sos_ragged_stage_f32, sos_ragged_unpack_f32,
sos_silence_label_batch and sos_silence_label_workspace_bytes answer to a table with one defect, and the table helpers of
ragged.py.  Every call below is refused on the host before anything is launched -- the pointers to device memory are dummies
that are never dereferenced, so no GPU is needed (tests/test_wave_io_batch_cpu.py checks the resampler the same way).  The
return codes, the entry named, the messages and the byte counts are those of the library before the three entry points moved
onto the shared helpers of ragged.h."""
import ctypes as C

import numpy as np
import pytest

_buf = (C.c_float * 64)()
P = C.cast(_buf, C.c_void_p)                     # stands for every device pointer


def _host(a):
    return a.ctypes.data_as(C.c_void_p)


def _answer(rc):
    from sos_amd import _lib as L
    return rc, L.lib().sos_last_error().decode()


def _refused(rc_msg, fn, rc, *fragments):
    got, msg = rc_msg
    assert got == rc, (got, msg)
    assert msg.startswith(fn + ":"), msg
    for f in fragments:
        assert f in msg, (f, msg)


# ---------------------------------------------------------------------------------------------- sos_ragged_stage_f32
STAGE_NS, STAGE_NB = [257, 1, 4097], [1, 34, 8]


def _stage(tab, nclips=3, stride=4100, ratios=(466.0, 466.0, 466.0)):
    from sos_amd import _lib as L
    rat = np.asarray(ratios, dtype=np.float64)
    return _answer(L.lib().sos_ragged_stage_f32(P, P, _host(tab), nclips, P, P, _host(rat), stride, P, P, P, None))


def _defect(ns, nb, row=None, col=None, value=None, add=None):
    from sos_amd import ragged
    tab = ragged.clip_table(ns, nb)
    if row is not None:
        tab[row, col] = tab[row, col] + add if add is not None else value
    return tab


@pytest.mark.parametrize("edit,kwargs,fragments", [
    (dict(row=2, col=0, add=1), {}, ["clip 2 (samples 259 + 4097, frames 35 + 8) lies outside the 4355 samples / 43 frames"]),
    (dict(row=2, col=2, add=1), {}, ["clip 2 (samples 258 + 4097, frames 36 + 8) lies outside"]),
    (dict(row=1, col=1, value=-1), {}, ["clip 1 has -1 samples (stride 4100) and 34 frames"]),
    (dict(row=1, col=3, value=-1), {}, ["clip 1 has 1 samples (stride 4100) and -1 frames"]),
    ({}, dict(stride=4096), ["clip 2 has 4097 samples (stride 4096)"]),
    ({}, dict(nclips=0), ["1 .. 65535 clips, got 0"]),
    ({}, dict(nclips=65536), ["1 .. 65535 clips, got 65536"]),
    ({}, dict(ratios=(466.0, 1.0, 466.0)), ["clip 1 has ratio 1"]),
], ids=["sample-offset", "frame-offset", "samples<0", "frames<0", "stride", "no-clips", "too-many-clips", "ratio"])
def test_stage_refuses_one_defect_by_name(edit, kwargs, fragments):
    _refused(_stage(_defect(STAGE_NS, STAGE_NB, **edit), **kwargs), "sos_ragged_stage_f32", -22, *fragments)


# --------------------------------------------------------------------------------------------- sos_ragged_unpack_f32
@pytest.mark.parametrize("rows,stride,fragment", [
    ([(0, 1, 0), (5, 11200, 2)], 11200, "entry 1 (output 2 + 11200) lies outside the 11201 samples"),
    ([(6, 1, 0)], 11200, "entry 0 takes 1 samples of row 6 (6 rows of 11200)"),
    ([(0, 5, 0)], 4, "entry 0 takes 5 samples of row 0 (6 rows of 4)"),
], ids=["output-offset", "row", "stride"])
def test_unpack_refuses_one_defect_by_name(rows, stride, fragment):
    from sos_amd import _lib as L
    tab = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
    _refused(_answer(L.lib().sos_ragged_unpack_f32(P, 6, stride, P, _host(tab), len(rows), P, None)),
             "sos_ragged_unpack_f32", -22, fragment)


# ------------------------------------------------------------------------------------------- sos_silence_label_batch
LABEL_NS, LABEL_NB = [1400, 467, 4097], [3, 2, 9]
LABEL_TABLE_DEFECTS = [dict(row=2, col=0, add=1), dict(row=2, col=2, add=1), dict(row=1, col=1, value=0),
                       dict(row=1, col=3, value=3), dict(row=2, col=3, value=8)]


def _label(tab, par_edit=None, workspace_bytes=1 << 40):
    from sos_amd import _lib as L
    par = np.tile(np.asarray([14000 / 30, 1e-4, 0.0, 3.0, 1.0], dtype=np.float64), (3, 1))
    if par_edit is not None:
        par[1, par_edit[0]] = par_edit[1]
    return _answer(L.lib().sos_silence_label_batch(P, P, _host(tab), 3, P, _host(par), P, workspace_bytes, P, P, P, None))


@pytest.mark.parametrize("edit,fragments", list(zip(LABEL_TABLE_DEFECTS, [
    ["clip 2 (samples 1868 + 4097, frames 5 + 9) lies outside the 5964 samples / 14 frames"],
    ["clip 2 (samples 1867 + 4097, frames 6 + 9) lies outside"],
    ["clip 1 has 0 samples and 2 frames"],
    ["clip 1: 3 frames of 466.667 samples do not tile 467 samples (the last frame would be empty)"],
    ["clip 2: 8 frames", "4097 samples (samples would be left over)"],
])), ids=["sample-offset", "frame-offset", "samples=0", "frame-too-many", "frame-too-few"])
def test_labels_refuse_one_table_defect_by_name(edit, fragments):
    _refused(_label(_defect(LABEL_NS, LABEL_NB, **edit)), "sos_silence_label_batch", -22, *fragments)


@pytest.mark.parametrize("par_edit,fragment", [
    ((0, 1.0), "has ratio 1"),
    ((1, -1.0), "relative threshold -1"),
    ((3, 0.0), "minimum run lengths 0 (silent) and 1 (speech)"),
    ((2, float("nan")), "floor nan"),
], ids=["ratio", "rel", "min-silent", "floor"])
def test_labels_refuse_one_parameter_defect_by_name(par_edit, fragment):
    _refused(_label(_defect(LABEL_NS, LABEL_NB), par_edit), "sos_silence_label_batch", -22, "clip 1", fragment)


def test_labels_refuse_a_short_workspace():
    _refused(_label(_defect(LABEL_NS, LABEL_NB), workspace_bytes=8), "sos_silence_label_batch", -28,
             "workspace of 8 bytes, 512 needed")


# --------------------------------------------------------------------------------- sos_silence_label_workspace_bytes
def _workspace_bytes(tab, nclips=None):
    from sos_amd import _lib as L
    return L.lib().sos_silence_label_workspace_bytes(_host(tab) if tab is not None else None, len(tab) if nclips is None else nclips)


@pytest.mark.parametrize("frames,nbytes", [
    ([1], 512),
    ([300, 1, 645], 7680),
    (np.random.default_rng(11).integers(1, 2001, 300), 2382080),
], ids=["one-frame", "three-clips", "300-clips"])
def test_label_workspace_bytes_are_unchanged(frames, nbytes):
    from sos_amd import ragged
    frames = np.asarray(frames, dtype=np.int64)
    if len(frames) == 300:
        assert int(frames.sum()) == 297570
    assert _workspace_bytes(ragged.clip_table(467 * frames, frames)) == nbytes


@pytest.mark.parametrize("edit", LABEL_TABLE_DEFECTS, ids=["sample-offset", "frame-offset", "samples=0", "frame-too-many",
                                                           "frame-too-few"])
def test_label_workspace_bytes_of_a_table_the_launch_refuses(edit):
    """The sizer names no clip: it returns a size, and the launch refuses the table."""
    assert _workspace_bytes(_defect(LABEL_NS, LABEL_NB, **edit)) == 512


def test_label_workspace_bytes_refuse_a_bad_clip_count():
    tab = _defect(LABEL_NS, LABEL_NB)
    assert _workspace_bytes(tab, 0) == -1 and _workspace_bytes(tab, 65536) == -1 and _workspace_bytes(None, 3) == -1


# ------------------------------------------------------------------------------------------------------- ragged.py
def test_offsets_and_clip_table():
    from sos_amd import ragged
    for empty in (ragged.offsets([]), ragged.clip_table([]), ragged.clip_table([], [])):
        assert empty.dtype == np.int64 and empty.size == 0
    assert ragged.clip_table([]).shape == (0, 4)
    assert ragged.offsets([5]).tolist() == [0] and ragged.offsets(np.asarray([3, 0, 4], np.int32)).tolist() == [0, 3, 3]
    assert ragged.offsets([2 ** 40, 2 ** 40, 1]).tolist() == [0, 2 ** 40, 2 ** 41]          # int64 whatever the platform's int
    one = ragged.clip_table([7], [2])
    assert one.dtype == np.int64 and one.flags.c_contiguous and one.tolist() == [[0, 7, 0, 2]]
    tab = ragged.clip_table(STAGE_NS, STAGE_NB)
    assert tab.tolist() == [[0, 257, 0, 1], [257, 1, 1, 34], [258, 4097, 35, 8]]
    assert ragged.clip_table(STAGE_NS).tolist() == [[0, 257, 0, 0], [257, 1, 0, 0], [258, 4097, 0, 0]]
    assert ragged.MAX_CLIPS == 65535


def test_per_clip():
    from sos_amd import ragged
    v = ragged.per_clip(30, 3, "fps")
    assert v.dtype == np.float64 and v.tolist() == [30.0, 30.0, 30.0] and v.flags.writeable
    assert ragged.per_clip([25, 30.5], 2, "fps").tolist() == [25.0, 30.5]
    assert ragged.per_clip(np.float32(2.5), 1, "sr").tolist() == [2.5] and ragged.per_clip(7, 0, "sr").shape == (0,)
    for wrong in ([25, 30], [[25, 30, 24]], []):
        with pytest.raises(ValueError, match="fps"):
            ragged.per_clip(wrong, 3, "fps")


def test_split_returns_views_of_tensors_and_arrays():
    import torch
    from sos_amd import ragged
    lens = [3, 0, 1, 4]
    for flat in (np.arange(8, dtype=np.float32), torch.arange(8, dtype=torch.float32)):
        parts = ragged.split(flat, lens)
        assert [len(p) for p in parts] == lens and type(parts[0]) is type(flat)
        assert [float(v) for p in parts for v in p] == [float(v) for v in range(8)]
        parts[3][0] = -1.0                                       # a view: the write lands in `flat`
        assert float(flat[4]) == -1.0
        assert ragged.split(flat, []) == [] and len(ragged.split(flat, [8])[0]) == 8
    assert ragged.download([]) == []


def test_chunks_read_max_clips_when_called(monkeypatch):
    from sos_amd import ragged
    assert list(ragged.chunks(0)) == [] and list(ragged.chunks(65535)) == [(0, 65535)]
    assert list(ragged.chunks(65536)) == [(0, 65535), (65535, 65536)]
    monkeypatch.setattr("sos_amd.ragged.MAX_CLIPS", 3)
    assert list(ragged.chunks(7)) == [(0, 3), (3, 6), (6, 7)] and list(ragged.chunks(0)) == []
    assert list(ragged.chunks(3)) == [(0, 3)] and list(ragged.chunks(4)) == [(0, 3), (3, 4)]


def test_host_table_is_int64_c_contiguous_and_never_empty():
    from sos_amd import ragged
    rows = ragged.host_table([(0, 5, 1), (5, 2, 0)], 3)
    assert rows.dtype == np.int64 and rows.flags.c_contiguous and rows.tolist() == [[0, 5, 1], [5, 2, 0]]
    assert ragged.host_table(np.arange(6, dtype=np.int32), 2).tolist() == [[0, 1], [2, 3], [4, 5]]
    cols = ragged.host_table([np.asarray([0, 5]), [5, 2], np.asarray([1, 0], np.int32)])          # stacked columns keep their shape
    assert cols.dtype == np.int64 and cols.flags.c_contiguous and cols.tolist() == [[0, 5], [5, 2], [1, 0]]
    assert ragged.host_table(np.arange(6, dtype=np.int64).reshape(2, 3).T).flags.c_contiguous
    for empty, cols in (([], 4), ([], None), (np.zeros((6, 0), np.int64), None), (np.zeros((0, 4), np.int64), 4)):
        with pytest.raises(ValueError, match="an empty table"):
            ragged.host_table(empty, cols)


def test_group_by_and_per_group():
    """group_by gives the dict that recordings._resample_back built by hand; per_group runs one call per key and scatters."""
    from sos_amd import ragged
    SR, rates = 14000, [44100, 14000, 8000, 44100, 14000, 48000, 8000, 44100]
    by_rate = {}
    for k, r in enumerate(rates):
        if r != SR:
            by_rate.setdefault(r, []).append(k)
    got = ragged.group_by(rates, lambda k, r: r == SR)
    assert got == by_rate == {44100: [0, 3, 7], 8000: [2, 6], 48000: [5]} and list(got) == [44100, 8000, 48000]
    assert ragged.group_by(rates) == {44100: [0, 3, 7], 14000: [1, 4], 8000: [2, 6], 48000: [5]}
    assert ragged.group_by([]) == {} and ragged.group_by(rates, lambda k, r: True) == {}
    assert ragged.group_by("abca", lambda k, key: k == 0) == {"b": [1], "c": [2], "a": [3]}
    calls, items = [], ["x%d" % k for k in range(len(rates))]
    out = ragged.per_group(items, rates, lambda r, idx: calls.append((r, idx)) or ["%s@%d" % (items[k], r) for k in idx],
                           lambda k, r: r == SR)
    assert calls == [(44100, [0, 3, 7]), (8000, [2, 6]), (48000, [5])]
    assert out == ["x0@44100", "x1", "x2@8000", "x3@44100", "x4", "x5@48000", "x6@8000", "x7@44100"]
    assert items[0] == "x0" and out is not items                 # a copy: the items given stay


def test_back_to_back_is_a_view_of_split_outputs_and_a_copy_otherwise():
    import torch
    from sos_amd import ragged
    flat = torch.arange(12, dtype=torch.float32)
    parts = ragged.split(flat, [3, 0, 5, 4])
    whole = ragged.back_to_back(parts)
    assert whole.data_ptr() == flat.data_ptr() and whole.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
    assert torch.equal(whole, flat)
    tail = ragged.back_to_back(parts[2:])                        # off the buffer's start: still a view
    assert tail.data_ptr() == parts[2].data_ptr() and tail.storage_offset() == 3 and torch.equal(tail, flat[3:])
    planes = [p.view(1, -1) for p in parts[2:]]                  # 2-D planes that lie back to back
    assert ragged.back_to_back(planes).data_ptr() == parts[2].data_ptr() and ragged.back_to_back(planes).shape == (9,)
    for apart in ([parts[0], parts[3]], [parts[3], parts[2]], [parts[0].clone(), parts[2]], [flat[::2][:3], flat[6:]],
                  [parts[0], parts[2].double()]):
        got = ragged.back_to_back(apart)
        assert got.untyped_storage().data_ptr() != flat.untyped_storage().data_ptr()
        assert torch.equal(got, torch.cat([t.reshape(-1) for t in apart]))
    some = ragged.flat_f32([parts[1], parts[2], parts[1]], "cpu")
    assert some.data_ptr() == parts[2].data_ptr() and some.numel() == 5
    none = ragged.flat_f32([parts[1], parts[1]], "cpu")          # never a null pointer
    assert none.numel() == 1 and none.dtype == torch.float32 and float(none[0]) == 0.0
