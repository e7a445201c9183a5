"""What sos_pcm_encode_dither_batch (csrc/pcm_io.hip) and audio_io.encode_batch_device(dither=) / pcm_encode_device refuse.  Every
call below is refused on the host before anything is launched or uploaded -- the pointers to device memory are dummies that are
never dereferenced and the tensors live on the CPU -- so no GPU is needed (tests/test_pcm_host_cpu.py does the same for the
undithered entry points).  tests/test_gpu_dither.py runs these tests again beside the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

_buf = (C.c_float * 64)()
P = C.cast(_buf, C.c_void_p)                     # stands for every device pointer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, CHANNELS = [257, 1, 1025], [2, 1, 3]
S16, S32, F32, U8, S24, ALAW, ULAW = 0, 1, 2, 3, 4, 6, 7
TPDF, HIGHPASS = 1, 2
LIMIT = 1 << 62


def dither_table():
    """The encode rows {first plane sample, available, channels, frames, output element}, then {file key, frame0}: the largest
    key and the largest frame0 its file may have among them."""
    avail, frames = np.asarray(FRAMES, dtype=np.int64), np.asarray([200, 1, 1100], dtype=np.int64)
    src, dst = avail * CHANNELS, frames * CHANNELS
    return np.ascontiguousarray(np.stack([np.cumsum(src) - src, avail, CHANNELS, frames, np.cumsum(dst) - dst,
                                          [0, (1 << 32) - 1, 7], [3, LIMIT - 1, 1 << 34]], axis=1), dtype=np.int64)


def _call(tab=None, nfiles=3, fmt=S16, kind=TPDF, seed=5, null=None):
    from sos_amd import _lib as L
    tab = dither_table() if tab is None else tab
    a = dict(planes=P, table=P, table_host=tab.ctypes.data_as(C.c_void_p), out=P, clipped=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_pcm_encode_dither_batch(a["planes"], a["table"], a["table_host"], nfiles, fmt, kind, seed, a["out"], a["clipped"], None)
    return rc, h.sos_last_error().decode()


def _refused(got, *fragments):
    rc, msg = got
    assert rc == -22, (rc, msg)                                  # SOS_EINVAL
    assert msg.startswith("sos_pcm_encode_dither_batch:"), msg
    for f in fragments:
        assert f in msg, (f, msg)


def _edit(row, col, value):
    tab = dither_table()
    tab[row, col] = value
    return tab


def test_header_declares_and_both_libraries_export_the_symbol():
    import sos_amd
    from sos_amd import _lib as L
    from sos_amd import audio_io
    hdr = open(os.path.join(ROOT, "include", "sos_hip.h")).read()
    assert re.search(r"\bsos_pcm_encode_dither_batch\s*\(", hdr) and len(L.SIGNATURES["sos_pcm_encode_dither_batch"]) == 10
    assert re.search(r"enum\s*\{\s*SOS_DITHER_TPDF = 1, SOS_DITHER_HIGHPASS = 2\s*\}", hdr)
    assert audio_io.DITHER == dict(tpdf=TPDF, highpass=HIGHPASS) and audio_io.DITHER_FORMATS == ("u8", "s16", "s24")
    for precision in ("bf16", "fp16"):                           # the bfloat16 and the IEEE-half build
        sos_amd.set_precision(precision)
        try:
            h = L.lib()
        finally:
            sos_amd.set_precision("bf16")
        assert hasattr(h, "sos_pcm_encode_dither_batch") and h.sos_abi_version() == L.EXPECTED_ABI == 10


@pytest.mark.parametrize("kind", [0, 3, -1])
def test_c_refuses_another_kind(kind):
    _refused(_call(kind=kind), "unknown dither %d" % kind)


@pytest.mark.parametrize("fmt", [S32, F32, ALAW, ULAW])
def test_c_refuses_the_formats_without_dither(fmt):
    _refused(_call(fmt=fmt), "sample format %d takes no dither" % fmt)


def test_c_refuses_what_the_plain_encode_refuses():
    _refused(_call(fmt=5), "unknown sample format 5")
    _refused(_call(nfiles=0), "1 .. 65535 files, got 0")
    for name in ("planes", "table", "table_host", "out", "clipped"):
        _refused(_call(null=name), "null pointer")
    _refused(_call(tab=_edit(1, 2, 65)), "file 1", "channels outside 1 .. 64")
    _refused(_call(tab=_edit(2, 4, 402)), "file 2", "output element 402", "outside the totals")


@pytest.mark.parametrize("fmt", [S16, S24, U8])
@pytest.mark.parametrize("edit,fragments", [
    ((0, 5, -1), ["file 0", "dither key -1"]),
    ((2, 5, 1 << 32), ["file 2", "dither key 4294967296"]),
    ((1, 6, -1), ["file 1", "first frame -1"]),
    ((1, 6, LIMIT), ["file 1", "first frame %d" % LIMIT, "its 1 frames"]),
    ((2, 6, LIMIT - 1099), ["file 2", "its 1100 frames"]),
], ids=["key<0", "key=2^32", "frame0<0", "frame0=2^62", "frame0+frames>2^62"])
def test_c_refuses_a_key_or_first_frame_out_of_range(fmt, edit, fragments):
    _refused(_call(tab=_edit(*edit), fmt=fmt, kind=HIGHPASS), *fragments)


def _planes():
    import torch
    return [torch.zeros(2, 8), torch.zeros(1, 3)]               # on the CPU: a call that is not refused fails on that


@pytest.mark.parametrize("kwargs,match", [
    (dict(dither="rpdf"), "unknown dither 'rpdf'"),
    (dict(dither=1), "unknown dither 1"),
    (dict(fmt="s32"), "sample format 's32' takes no dither"),
    (dict(fmt="f32"), "sample format 'f32' takes no dither"),
    (dict(fmt="alaw"), "sample format 'alaw' takes no dither"),
    (dict(fmt="ulaw"), "sample format 'ulaw' takes no dither"),
    (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"), (dict(seed=1.5), "seed"), (dict(seed=True), "seed"),
    (dict(keys=[1]), "keys holds one integer per file"),
    (dict(keys=[0, -1]), r"keys\[1\] = -1"),
    (dict(keys=[1 << 32, 0]), r"keys\[0\] = 4294967296"),
    (dict(keys=[0.5, 0]), r"keys\[0\]"),
    (dict(frame0=[0, 0, 0]), "frame0 holds one integer per file"),
    (dict(frame0=[-1, 0]), r"frame0\[0\] = -1"),
    (dict(frame0=[0, LIMIT - 2]), r"frame0\[1\]"),              # 3 frames: at most 2^62 - 3
    (dict(frame0=[LIMIT - 7, 0], frames=[8, 3]), r"frame0\[0\]"),
], ids=lambda v: "-".join("%s" % k for k in v) if isinstance(v, dict) else None)
def test_python_refuses_before_any_launch(kwargs, match):
    from sos_amd import audio_io
    args = dict(fmt="s16", dither="tpdf", seed=1, keys=None, frame0=None, frames=None)
    args.update(kwargs)
    fmt = args.pop("fmt")
    with pytest.raises(ValueError, match=match):
        audio_io.encode_batch_device(_planes(), fmt, **args)


def test_python_accepts_the_ends_of_the_ranges_and_then_asks_for_the_gpu():
    """What is in range passes the argument checks; on CPU tensors the next thing is the refusal to run without a GPU."""
    from sos_amd import audio_io
    for kind in ("tpdf", "highpass"):
        with pytest.raises(RuntimeError, match="MI355X"):
            audio_io.encode_batch_device(_planes(), "s24", dither=kind, seed=(1 << 64) - 1, keys=[(1 << 32) - 1, 0],
                                         frame0=[LIMIT - 8, np.int64(0)])


def test_the_packet_form_checks_its_own_arguments():
    import torch
    from sos_amd import audio_io
    with pytest.raises(ValueError, match="unsupported sample format 'alaw'"):
        audio_io.pcm_encode_device(torch.zeros(4), "alaw")
    with pytest.raises(ValueError, match="1-D float32"):
        audio_io.pcm_encode_device(torch.zeros(1, 4), "s16")
    with pytest.raises(ValueError, match="takes no dither"):
        audio_io.pcm_encode_device(torch.zeros(4), "s32", dither="tpdf")
    with pytest.raises(ValueError, match=r"keys\[0\]"):
        audio_io.pcm_encode_device(torch.zeros(4), "s16", dither="tpdf", key=-1)
    with pytest.raises(ValueError, match=r"frame0\[0\]"):
        audio_io.pcm_encode_device(torch.zeros(4), "s16", dither="tpdf", frame0=LIMIT - 3)


def test_denoise_recordings_refuses_its_dither_arguments_first():
    from sos_amd import recordings
    with pytest.raises(ValueError, match="unknown dither 'white'"):
        recordings.denoise_recordings(None, None, ["missing.wav"], "out", dither="white")
    for seed in (-1, 1 << 64, 0.5, True):
        with pytest.raises(ValueError, match="dither_seed"):
            recordings.denoise_recordings(None, None, ["missing.wav"], "out", dither="tpdf", dither_seed=seed)
