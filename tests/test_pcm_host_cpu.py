"""The host half of sos_pcm_planes_batch_f32 / sos_pcm_encode_batch (csrc/pcm_io.hip) and the argument checks of
audio_io.decode_planes_batch_device / encode_batch_device.  Every call below is refused on the host before anything is launched
or uploaded -- the pointers to device memory are dummies that are never dereferenced, so no GPU is needed
(tests/test_ragged_mix_host_cpu.py does the same for the mixer)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

_buf = (C.c_float * 64)()
P = C.cast(_buf, C.c_void_p)                     # stands for every device pointer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, CHANNELS = [257, 1, 1025], [2, 1, 3]


def _host(a):
    return a.ctypes.data_as(C.c_void_p)


def planes_table():
    """{pcm element offset, frames, channels, first output sample} of three files back to back."""
    n = np.asarray(FRAMES, dtype=np.int64) * CHANNELS
    off = np.cumsum(n) - n
    return np.ascontiguousarray(np.stack([off, FRAMES, CHANNELS, off], axis=1), dtype=np.int64)


def encode_table():
    """{first plane sample, available, channels, frames to write, output element offset}: cropped, equal, zero-filled."""
    avail, frames = np.asarray(FRAMES, dtype=np.int64), np.asarray([200, 1, 1100], dtype=np.int64)
    src, dst = avail * CHANNELS, frames * CHANNELS
    return np.ascontiguousarray(np.stack([np.cumsum(src) - src, avail, CHANNELS, frames, np.cumsum(dst) - dst], axis=1), dtype=np.int64)


def _planes(tab=None, nfiles=3, fmt=0, null=None):
    from sos_amd import _lib as L
    tab = planes_table() if tab is None else tab
    a = dict(pcm=P, table=P, table_host=_host(tab), out=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_pcm_planes_batch_f32(a["pcm"], fmt, a["table"], a["table_host"], nfiles, a["out"], None)
    return rc, h.sos_last_error().decode(), "sos_pcm_planes_batch_f32:"


def _encode(tab=None, nfiles=3, fmt=0, null=None):
    from sos_amd import _lib as L
    tab = encode_table() if tab is None else tab
    a = dict(planes=P, table=P, table_host=_host(tab), out=P, clipped=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_pcm_encode_batch(a["planes"], a["table"], a["table_host"], nfiles, fmt, a["out"], a["clipped"], None)
    return rc, h.sos_last_error().decode(), "sos_pcm_encode_batch:"


def _refused(got, *fragments):
    rc, msg, who = got
    assert rc == -22, (rc, msg)                                  # SOS_EINVAL
    assert msg.startswith(who), msg
    for f in fragments:
        assert f in msg, (f, msg)


def _edit(make, row, col, value):
    tab = make()
    tab[row, col] = value
    return tab


def test_header_declares_and_library_exports_the_two_symbols():
    from sos_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sos_hip.h")).read()
    h = L.lib()
    for name, nargs in (("sos_pcm_planes_batch_f32", 7), ("sos_pcm_encode_batch", 8)):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(h, name) and len(L.SIGNATURES[name]) == nargs
    m = re.search(r"enum\s*\{\s*SOS_ENC_S16 = 0, SOS_ENC_S32 = 1, SOS_ENC_F32 = 2, SOS_ENC_U8 = 3, SOS_ENC_S24 = 4\s*\}", hdr)
    assert m, "the encode formats extend SOS_PCM_* by packed s24"
    from sos_amd import audio_io
    assert {k: v[0] for k, v in audio_io.ENCODINGS.items()} == dict(s16=0, s32=1, f32=2, u8=3, s24=4)
    assert h.sos_abi_version() == L.EXPECTED_ABI == 10          # an added symbol breaks no caller


@pytest.mark.parametrize("name", ["pcm", "table", "table_host", "out"])
def test_decode_refuses_a_null_pointer(name):
    _refused(_planes(null=name), "null pointer")


@pytest.mark.parametrize("name", ["planes", "table", "table_host", "out", "clipped"])
def test_encode_refuses_a_null_pointer(name):
    _refused(_encode(null=name), "null pointer")


@pytest.mark.parametrize("call", [_planes, _encode], ids=["decode", "encode"])
def test_file_counts_and_formats_are_refused(call):
    _refused(call(nfiles=0), "1 .. 65535 files, got 0")
    _refused(call(nfiles=65536), "1 .. 65535 files, got 65536")        # refused before the table is read
    _refused(call(fmt=5), "unknown sample format 5")
    _refused(call(fmt=-1), "unknown sample format -1")


def test_decode_has_no_packed_s24():
    """24-bit files are carried as s32 (audio_io.read_wave); SOS_ENC_S24 = 4 is an encode format only."""
    _refused(_planes(fmt=4), "unknown sample format 4")


@pytest.mark.parametrize("edit,fragments", [
    ((1, 2, 0), ["file 1", "channels outside 1 .. 64"]),
    ((2, 2, 65), ["file 2", "65 channels", "channels outside 1 .. 64"]),
    ((0, 1, -1), ["file 0", "-1 frames", "negative or too large"]),
    ((1, 1, 1 << 62), ["file 1", "negative or too large"]),
    ((2, 0, 516), ["file 2 (pcm element 516, 1025 frames, 3 channels, output 515)", "outside the totals", "3590 elements"]),
    ((2, 3, 516), ["file 2", "output 516", "outside the totals"]),
    ((0, 0, -2), ["file 0 (pcm element -2", "outside the totals"]),
], ids=["channels=0", "channels=65", "frames<0", "frames-huge", "pcm-past-the-end", "out-past-the-end", "offset<0"])
def test_decode_refuses_one_bad_row_by_file(edit, fragments):
    _refused(_planes(tab=_edit(planes_table, *edit)), *fragments)


@pytest.mark.parametrize("edit,fragments", [
    ((1, 2, 0), ["file 1", "channels outside 1 .. 64"]),
    ((0, 2, 65), ["file 0", "65 channels"]),
    ((2, 1, -5), ["file 2", "-5 available", "negative or too large"]),
    ((0, 3, -1), ["file 0", "-1 frames", "negative or too large"]),
    ((2, 0, 516), ["file 2 (plane sample 516, 1025 available", "outside the totals", "3590 plane samples"]),
    ((2, 4, 402), ["file 2", "output element 402", "outside the totals", "3701 output elements"]),
    ((1, 4, -1), ["file 1", "output element -1", "outside the totals"]),
], ids=["channels=0", "channels=65", "available<0", "frames<0", "planes-past-the-end", "out-past-the-end", "out<0"])
def test_encode_refuses_one_bad_row_by_file(edit, fragments):
    _refused(_encode(tab=_edit(encode_table, *edit)), *fragments)


@pytest.mark.parametrize("kwargs,match", [
    (dict(kinds=["s16"]), "one kind per array"),
    (dict(kinds=["s16", "s24"]), r"file 1 has the unsupported sample format 's24'"),
    (dict(arrs=[np.zeros((4, 2), np.int16), np.zeros(4, np.int16)]), "file 1 must be"),
    (dict(arrs=[np.zeros((4, 0), np.int16), np.zeros((4, 1), np.int16)]), "file 0 must be"),
    (dict(arrs=[np.zeros((4, 2), np.int16), np.zeros((4, 65), np.int16)]), "file 1 must be"),
])
def test_decode_argument_errors_are_raised_without_a_gpu(kwargs, match):
    from sos_amd import audio_io
    args = dict(arrs=[np.zeros((4, 2), np.int16), np.zeros((3, 1), np.int16)], kinds=["s16", "s16"])
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        audio_io.decode_planes_batch_device(**args)


def test_encode_argument_errors_are_raised_without_a_gpu():
    import torch
    from sos_amd import audio_io
    with pytest.raises(ValueError, match="unsupported sample format 'f64'"):
        audio_io.encode_batch_device([torch.zeros(1, 4)], "f64")
    with pytest.raises(ValueError, match="file 1 must be"):
        audio_io.encode_batch_device([torch.zeros(1, 4), torch.zeros(4)], "s16")
    with pytest.raises(ValueError, match="file 0 must be"):
        audio_io.encode_batch_device([torch.zeros(65, 4)], "s16")
    with pytest.raises(ValueError, match="file 0 must be"):
        audio_io.encode_batch_device([torch.zeros(1, 4, dtype=torch.float64)], "s16")
    with pytest.raises(RuntimeError, match="MI355X"):                  # no CPU fallback
        audio_io.encode_batch_device([torch.zeros(1, 4)], "s16")


def test_mono_false_keeps_raising():
    from sos_amd import audio_io
    with pytest.raises(NotImplementedError):
        audio_io.load_device("x.wav", mono=False)
    with pytest.raises(NotImplementedError):
        audio_io.load_batch_device(["x.wav"], mono=False)
