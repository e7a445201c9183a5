"""The host half of sos_band_gain_batch_f32 / sos_resample_merge_batch_f32 (csrc/band_merge.hip), the argument checks of
audio_io.band_gains_batch_device / resample_merge_batch_device and of recordings.denoise_recordings(high_band=, smooth_frames=).
Every call below is refused on the host before anything is launched or uploaded -- the pointers to device memory are dummies that
are never dereferenced, so no GPU is needed (tests/test_pcm_host_cpu.py does the same for the channel planes).
Not reachable from here: SOS_ENOSPC.  The time register of a clip runs up to m <= 2^52, which sos_resample_time_segments
describes in 105 segments of the 120 the kernel argument holds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

_buf = (C.c_float * 64)()
P = C.cast(_buf, C.c_void_p)                     # stands for every device pointer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO, HOP, NWIN, NUM_TABLE, CHUNK = 48000.0 / 14000.0, 158, 32769, 512, 4096
N = [513, 4097, 9001]
M = [int(np.ceil(n / RATIO)) for n in N]         # 150, 1195, 2626
MP = [100, 1106, 2528]
J = [-(-m // HOP) for m in M]                    # 1, 8, 17


def _host(a):
    return a.ctypes.data_as(C.c_void_p)


def _off(v):
    v = np.asarray(v, dtype=np.int64)
    return np.cumsum(v) - v


def merge_table():
    """[9][3]: x / out offset, n, a offset, m, b offset, m', gains offset, J, first tile."""
    return np.ascontiguousarray(np.stack([_off(N), N, _off(M), M, _off(MP), MP, _off(J), J, _off([-(-n // CHUNK) for n in N])]),
                                dtype=np.int64)


def gain_table():
    """[6][3]: a offset, m, b offset, m', gains offset, J; the second clip has no output at all."""
    mp = [MP[0], 0, MP[2]]
    return np.ascontiguousarray(np.stack([_off(M), M, _off(mp), mp, _off(J), J]), dtype=np.int64)


def _merge(tab=None, nclips=3, ratio=RATIO, nwin=NWIN, hop=HOP, null=None, gains=True):
    from sos_amd import _lib as L
    tab = merge_table() if tab is None else tab
    a = dict(x=P, a=P, b=P, gains=P if gains else None, table=P, table_host=_host(tab), win=P, out=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_resample_merge_batch_f32(a["x"], a["a"], a["b"], a["gains"], a["table"], a["table_host"], nclips, ratio, a["win"], nwin,
                                        NUM_TABLE, hop, a["out"], None)
    return rc, h.sos_last_error().decode(), "sos_resample_merge_batch_f32:"


def _gain(tab=None, nclips=3, hop=HOP, smooth=2, null=None):
    from sos_amd import _lib as L
    tab = gain_table() if tab is None else tab
    a = dict(a=P, b=P, table=P, table_host=_host(tab), gains=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_band_gain_batch_f32(a["a"], a["b"], a["table"], a["table_host"], nclips, hop, smooth, a["gains"], None)
    return rc, h.sos_last_error().decode(), "sos_band_gain_batch_f32:"


def _refused(got, *fragments):
    rc, msg, who = got
    assert rc == -22, (rc, msg)                                  # SOS_EINVAL
    assert msg.startswith(who), msg
    for f in fragments:
        assert f in msg, (f, msg)


def _edit(make, row, clip, value):
    tab = make()
    tab[row, clip] = value
    return tab


def test_header_declares_and_library_exports_the_two_symbols():
    from sos_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sos_hip.h")).read()
    h = L.lib()
    for name, nargs in (("sos_band_gain_batch_f32", 9), ("sos_resample_merge_batch_f32", 14)):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(h, name) and len(L.SIGNATURES[name]) == nargs
    assert "fmaf(g[t], x[t] - U(a)[t], U(b)[t])" in hdr, "the header states the rule"
    assert h.sos_abi_version() == L.EXPECTED_ABI == 10          # an added symbol breaks no caller


@pytest.mark.parametrize("name", ["x", "a", "b", "table", "table_host", "win", "out"])
def test_merge_refuses_a_null_pointer(name):
    _refused(_merge(null=name), "null pointer")


@pytest.mark.parametrize("name", ["a", "b", "table", "table_host", "gains"])
def test_gains_refuse_a_null_pointer(name):
    _refused(_gain(null=name), "null pointer")


@pytest.mark.parametrize("call", [_merge, _gain], ids=["merge", "gains"])
def test_clip_counts_and_hop_are_refused(call):
    _refused(call(nclips=0), "1 .. 65535 clips, got 0")
    _refused(call(nclips=65536), "1 .. 65535 clips, got 65536")         # refused before the table is read
    _refused(call(hop=0), "hop=0")
    _refused(call(hop=-3), "hop=-3")


def test_merge_refuses_bad_scalars():
    _refused(_merge(ratio=0.0), "ratio=0")
    _refused(_merge(ratio=-1.0), "ratio=-1")
    _refused(_merge(ratio=float("nan")), "nan")
    _refused(_merge(nwin=40960), "nwin=40960", "160 KB")
    _refused(_merge(nwin=1), "nwin=1")
    _refused(_merge(ratio=1e-4), "too small for a 512-point table")


def test_gains_refuse_a_smoothing_outside_0_to_16():
    _refused(_gain(smooth=-1), "smooth=-1", "0 .. 16")
    _refused(_gain(smooth=17), "smooth=17", "0 .. 16")


@pytest.mark.parametrize("edit,fragments", [
    ((1, 0, 0), ["clip 0 has n=0"]),
    ((3, 1, 0), ["clip 1 has n=4097, m=0"]),
    ((5, 2, 0), ["clip 2 has n=9001, m=2626, m'=0"]),
    ((5, 1, 1196), ["clip 1", "m=1195, m'=1196", "m' at most m"]),
    ((1, 1, 4098), ["clip 1 has n=4098 frames", "m=1195 low-rate samples cover 4097"]),
    ((7, 2, 16), ["clip 2 has 16 gains", "17 expected"]),
    ((0, 1, 512), ["clip 1 overlaps its predecessor or is out of order", "x 512"]),
    ((2, 2, 1344), ["clip 2 overlaps", "a 1344"]),
    ((4, 1, 99), ["clip 1 overlaps", "b 99"]),
    ((6, 1, 0), ["clip 1 overlaps", "gains 0"]),
    ((8, 2, 2), ["clip 2", "first tile 2 where 3 is expected"]),
    ((0, 0, -1), ["clip 0 overlaps", "x -1"]),
    ((1, 0, 1 << 53), ["clip 0 has n=9007199254740992"]),
], ids=["n=0", "m=0", "m'=0", "m'>m", "not-covered", "J", "x-overlap", "a-overlap", "b-overlap", "gains-overlap", "tile", "x<0", "n-huge"])
def test_merge_refuses_one_bad_row_by_clip(edit, fragments):
    _refused(_merge(tab=_edit(merge_table, *edit)), *fragments)


def test_merge_without_gains_does_not_read_the_gain_rows():
    """gains == NULL: rows [6] and [7] may hold anything; the next refusal is another one."""
    tab = merge_table()
    tab[6], tab[7] = -5, 0
    tab[8, 2] = 7
    _refused(_merge(tab=tab, gains=False), "clip 2", "first tile 7 where 3 is expected")


@pytest.mark.parametrize("edit,fragments", [
    ((1, 0, 0), ["clip 0 has m=0"]),
    ((3, 2, -1), ["clip 2 has m=2626, m'=-1"]),
    ((3, 0, 151), ["clip 0 has m=150, m'=151", "m' within 0 .. m"]),
    ((5, 1, 7), ["clip 1 has 7 frames", "m=1195, hop=158: 8 expected"]),
    ((0, 1, 149), ["clip 1 overlaps its predecessor or is out of order", "a 149"]),
    ((2, 2, 99), ["clip 2 overlaps", "b 99"]),
    ((4, 2, 8), ["clip 2 overlaps", "gains 8"]),
], ids=["m=0", "m'<0", "m'>m", "J", "a-overlap", "b-overlap", "gains-overlap"])
def test_gains_refuse_one_bad_row_by_clip(edit, fragments):
    _refused(_gain(tab=_edit(gain_table, *edit)), *fragments)


def _t(n, dtype=None):
    import torch
    return torch.zeros(n, dtype=dtype or torch.float32)


def test_merge_argument_errors_are_raised_without_a_gpu():
    import torch
    from sos_amd import audio_io
    x, a, b = [_t(513), _t(4097)], [_t(150), _t(1195)], [_t(100), _t(1106)]
    with pytest.raises(ValueError, match="target_sr .* must exceed orig_sr"):
        audio_io.resample_merge_batch_device(x, a, b, 48000, 14000)
    with pytest.raises(ValueError, match="must exceed"):
        audio_io.resample_merge_batch_device(x, a, b, 14000, 14000)
    with pytest.raises(ValueError, match="2 natives, 1 low-rate inputs"):
        audio_io.resample_merge_batch_device(x, a[:1], b, 14000, 48000)
    with pytest.raises(ValueError, match="2 inputs, 1 outputs"):
        audio_io.resample_merge_batch_device(x, a, b[:1], 14000, 48000)
    with pytest.raises(ValueError, match="1 gains"):
        audio_io.resample_merge_batch_device(x, a, b, 14000, 48000, gains=[_t(1)])
    with pytest.raises(ValueError, match="clip 1: the networks' output has 1196 samples for an input of 1195"):
        audio_io.resample_merge_batch_device(x, a, [b[0], _t(1196)], 14000, 48000)
    with pytest.raises(ValueError, match="clip 0: the networks' output has 0 samples"):
        audio_io.resample_merge_batch_device(x, a, [_t(0), b[1]], 14000, 48000)
    with pytest.raises(ValueError, match="clip 1: expects 1-D float32"):
        audio_io.resample_merge_batch_device(x, a, [b[0], _t(1106, torch.float64)], 14000, 48000)
    with pytest.raises(ValueError, match="clip 0: expects 1-D float32"):
        audio_io.resample_merge_batch_device([torch.zeros(1, 513), x[1]], a, b, 14000, 48000)
    with pytest.raises(ValueError, match="clip 1: 4098 frames at 48000 Hz are not covered by 1195 samples"):
        audio_io.resample_merge_batch_device([x[0], _t(4098)], a, b, 14000, 48000)
    with pytest.raises(ValueError, match=r"clip 1: gains must be .* ceil\(1195 / 158\) = 8 values"):
        audio_io.resample_merge_batch_device(x, a, b, 14000, 48000, gains=[_t(1), _t(7)])
    with pytest.raises(ValueError, match="res_type"):
        audio_io.resample_merge_batch_device(x, a, b, 14000, 48000, res_type="kaiser_fast")
    with pytest.raises(RuntimeError, match="MI355X"):                  # no CPU fallback
        audio_io.resample_merge_batch_device(x, a, b, 14000, 48000)
    with pytest.raises(RuntimeError, match="MI355X"):
        audio_io.resample_merge_batch_device(x, a, b, 14000, 48000, gains=[_t(1), _t(8)])


def test_gains_argument_errors_are_raised_without_a_gpu():
    import torch
    from sos_amd import audio_io
    a, b = [_t(150), _t(1195)], [_t(0), _t(1106)]
    with pytest.raises(ValueError, match="2 inputs, 1 outputs"):
        audio_io.band_gains_batch_device(a, b[:1])
    with pytest.raises(ValueError, match="clip 0: the networks' output has 151 samples for an input of 150"):
        audio_io.band_gains_batch_device(a, [_t(151), b[1]])
    with pytest.raises(ValueError, match="clip 1: expects 1-D float32"):
        audio_io.band_gains_batch_device(a, [b[0], _t(1106, torch.int32)])
    with pytest.raises(ValueError, match="clip 0: the networks' output has 0 samples for an input of 0"):
        audio_io.band_gains_batch_device([_t(0), a[1]], b)
    with pytest.raises(ValueError, match="smooth_frames within 0 .. 16"):
        audio_io.band_gains_batch_device(a, b, smooth_frames=17)
    with pytest.raises(ValueError, match="hop is at least 1"):
        audio_io.band_gains_batch_device(a, b, hop=0)
    with pytest.raises(RuntimeError, match="MI355X"):                  # no CPU fallback
        audio_io.band_gains_batch_device(a, b)


@pytest.mark.parametrize("kwargs,match", [
    (dict(high_band="up"), "unknown high_band 'up'"),
    (dict(high_band=None), "unknown high_band None"),
    (dict(high_band="follow", smooth_frames=17), "smooth_frames"),
    (dict(high_band="follow", smooth_frames=-1), "smooth_frames"),
    (dict(smooth_frames=1.5), "smooth_frames"),
])
def test_denoise_recordings_refuses_the_arguments_before_anything_is_read_or_created(tmp_path, kwargs, match):
    """No file is opened (the path does not exist) and out_dir is not created: the refusal comes first, as for link_channels."""
    from sos_amd import recordings
    out_dir = tmp_path / "out"
    with pytest.raises(ValueError, match=match):
        recordings.denoise_recordings(None, None, [str(tmp_path / "missing.wav")], str(out_dir), **kwargs)
    assert not out_dir.exists()
