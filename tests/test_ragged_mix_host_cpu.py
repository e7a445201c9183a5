"""The host half of sos_ragged_mix_f32 / sos_ragged_mix_workspace_bytes (csrc/ragged_mix.hip) and the argument checks of
tools.add_signals_ragged.  Every call below is refused on the host before anything is launched or uploaded -- the pointers to
device memory are dummies that are never dereferenced, so no GPU is needed (tests/test_ragged_host_cpu.py does the same for the
other ragged entry points)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

_buf = (C.c_float * 64)()
P = C.cast(_buf, C.c_void_p)                     # stands for every device pointer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, NB = [257, 1, 4097], [1, 34, 8]
NOISE_TOTAL = 5000
ARGS = ("clips", "table", "table_host", "noise", "noise_table", "noise_table_host", "bits", "params", "params_host", "workspace",
        "mixed", "clean", "noise_out", "out")


def _host(a):
    return a.ctypes.data_as(C.c_void_p)


def _call(tab=None, ntab=None, par=None, nclips=3, null=None, workspace_bytes=1 << 40, noise_total=NOISE_TOTAL, norm=0.5):
    from sos_amd import _lib as L
    from sos_amd import ragged
    tab = ragged.clip_table(NS, NB) if tab is None else tab
    ntab = np.asarray([[0, 257], [4999, 1], [3, 4097]], dtype=np.int64) if ntab is None else ntab
    par = np.asarray([[3.0, 466.0], [-10.0, 0.0], [7.0, 560.0]], dtype=np.float64) if par is None else par
    a = dict(clips=P, table=P, table_host=_host(tab), noise=P, noise_table=P, noise_table_host=_host(ntab), bits=P, params=P,
             params_host=_host(par), workspace=P, mixed=P, clean=P, noise_out=P, out=P)
    if null is not None:
        a[null] = None
    h = L.lib()
    rc = h.sos_ragged_mix_f32(a["clips"], a["table"], a["table_host"], nclips, a["noise"], noise_total, a["noise_table"],
                              a["noise_table_host"], a["bits"], a["params"], a["params_host"], norm, a["workspace"],
                              workspace_bytes, a["mixed"], a["clean"], a["noise_out"], a["out"], None)
    return rc, h.sos_last_error().decode()


def _refused(rc_msg, rc, *fragments):
    got, msg = rc_msg
    assert got == rc, (got, msg)
    assert msg.startswith("sos_ragged_mix_f32:"), msg
    for f in fragments:
        assert f in msg, (f, msg)


def _edit(which, row, col, value):
    from sos_amd import ragged
    tab = ragged.clip_table(NS, NB)
    ntab = np.asarray([[0, 257], [4999, 1], [3, 4097]], dtype=np.int64)
    par = np.asarray([[3.0, 466.0], [-10.0, 0.0], [7.0, 560.0]], dtype=np.float64)
    dict(tab=tab, ntab=ntab, par=par)[which][row, col] = value
    return dict(tab=tab, ntab=ntab, par=par)


def test_header_declares_and_library_exports_the_two_symbols():
    from sos_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sos_hip.h")).read()
    h = L.lib()
    for name in ("sos_ragged_mix_workspace_bytes", "sos_ragged_mix_f32"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(h, name) and name in L.SIGNATURES
    m = re.search(r"#define\s+SOS_MIX_CHUNK\s+(\d+)", hdr)
    assert m and int(m.group(1)) == L.MIX_CHUNK == 4096
    assert h.sos_abi_version() == 10


def test_a_sound_call_over_dummy_pointers_is_only_short_of_workspace():
    """The tables of this file are sound: with a workspace of 8 bytes the call gets as far as the size check."""
    _refused(_call(workspace_bytes=8), -28, "workspace of 8 bytes, 768 needed")


@pytest.mark.parametrize("name", [a for a in ARGS if a != "bits"])
def test_a_null_pointer_is_refused(name):
    _refused(_call(null=name), -22, "null pointer")


@pytest.mark.parametrize("edit,fragments", [
    (("tab", 1, 1, 0), ["clip 1 has 0 samples (at least 1)"]),
    (("tab", 2, 0, 259), ["clip 2 (samples 259 + 4097) lies outside the 4355 samples"]),
    (("tab", 2, 2, 36), ["clip 2 (frames 36 + 8) lies outside the 43 frames"]),
    (("ntab", 0, 1, 258), ["clip 0", "noise crop 0 + 258", "no longer than the clip's 257 samples"]),
    (("ntab", 2, 0, 904), ["clip 2", "noise crop 904 + 4097 must lie inside the 5000 noise samples"]),
    (("ntab", 1, 0, -1), ["clip 1", "noise crop -1 + 1"]),
    (("par", 0, 1, 1.0), ["clip 0 has ratio 1 "]),
    (("par", 2, 1, 0.5), ["clip 2 has ratio 0.5"]),
    (("par", 1, 1, -3.0), ["clip 1 has ratio -3"]),
    (("par", 1, 0, float("nan")), ["clip 1 has snr nan"]),
], ids=["samples=0", "sample-offset", "frame-offset", "nz>n", "crop-past-the-noise", "noff<0", "ratio=1", "ratio<1", "ratio<0",
        "snr-nan"])
def test_one_defect_is_refused_by_clip(edit, fragments):
    _refused(_call(**_edit(*edit)), -22, *fragments)


def test_frames_of_a_clip_without_decisions_are_not_looked_at():
    """ratio 0: the clip's frame columns play no part (clip 1's frame offset is moved outside; the call reaches the size check)."""
    _refused(_call(workspace_bytes=8, **_edit("tab", 1, 2, 40)), -28, "workspace")


def test_bits_may_be_null_only_when_every_ratio_is_zero():
    _refused(_call(null="bits"), -22, "clip 0 has ratio 466 but bits is null")
    par = np.asarray([[3.0, 0.0], [-10.0, 0.0], [7.0, 0.0]], dtype=np.float64)
    _refused(_call(null="bits", par=par, workspace_bytes=8), -28, "workspace")


def test_bad_counts_and_norm_are_refused():
    _refused(_call(nclips=0), -22, "1 .. 65535 clips, got 0")
    _refused(_call(nclips=65536), -22, "1 .. 65535 clips, got 65536")
    _refused(_call(noise_total=-1), -22, "-1 noise samples")
    _refused(_call(norm=float("inf")), -22, "norm inf")


def _workspace_bytes(ns, nclips=None):
    from sos_amd import _lib as L
    from sos_amd import ragged
    tab = ragged.clip_table(ns)
    return L.lib().sos_ragged_mix_workspace_bytes(_host(tab), len(tab) if nclips is None else nclips)


def test_workspace_bytes():
    from sos_amd import _lib as L
    from sos_amd import ragged
    tab = ragged.clip_table(NS)
    h = L.lib()
    assert h.sos_ragged_mix_workspace_bytes(_host(tab), 0) == -1 and h.sos_ragged_mix_workspace_bytes(_host(tab), 65536) == -1
    assert h.sos_ragged_mix_workspace_bytes(None, 3) == -1
    # nclips int64, then 2 and 1 f64 per chunk, each array to 256 bytes: 1 + 1 + 2 chunks
    assert _workspace_bytes(NS) == 256 + 256 + 256
    assert _workspace_bytes([1]) == 768 and _workspace_bytes([4096]) == 768 and _workspace_bytes([4097 + 16 * 4096]) == 256 + 512 + 256
    sizes = [_workspace_bytes([n, 5, 3 * n]) for n in (1, 4096, 4097, 50000, 10 ** 6, 10 ** 8)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]                      # monotone in the lengths
    assert _workspace_bytes([4097, 0]) == 256 + 256 + 256                       # a clip the launch refuses by name counts as 0


@pytest.mark.parametrize("kwargs,match", [
    (dict(signals=[np.zeros((2, 3), np.float32)]), r"signals\[0\]"),
    (dict(signals=[np.zeros(5, np.int16)]), r"signals\[0\]"),
    (dict(signals=[np.zeros(5, np.float32), np.zeros(0, np.float32)], noises=[np.zeros(9, np.float32)] * 2), r"signals\[1\] is empty"),
    (dict(noises=[np.zeros((1, 9), np.float32)], noise_index=[0, 0]), r"noises\[0\]"),
    (dict(noises=[np.zeros(9, np.float32)]), "noise_index=None"),
    (dict(noises=[np.zeros(9, np.float32)], noise_index=[0]), "noise_index: one entry per clip"),
    (dict(noises=[np.zeros(9, np.float32)], noise_index=[0, 1]), "outside the 1 noises"),
    (dict(noises=[np.zeros(9, np.float32)], noise_index=[0, -1]), "outside the 1 noises"),
    (dict(starts=[0, -1]), "non-negative"),
    (dict(starts=[0, 1, 2]), "starts"),
    (dict(counts=[1]), "counts"),
    (dict(counts=-2), "non-negative"),
    (dict(snr=[1.0, 2.0, 3.0]), "snr"),
    (dict(snr=float("nan")), "snr must be finite"),
    (dict(bits=[np.ones(3, np.uint8)], ratios=466.0), "bits: one entry"),
    (dict(bits=[np.ones(3, np.float32), None], ratios=466.0), r"bits\[0\]"),
    (dict(bits=[np.ones((3, 1), np.uint8), None], ratios=466.0), r"bits\[0\]"),
    (dict(bits=[None, np.ones(3, np.uint8)]), r"ratios\[1\]"),
    (dict(bits=[None, np.ones(3, np.uint8)], ratios=[None, 1.0]), r"ratios\[1\]"),
    (dict(bits=[None, np.ones(3, np.uint8)], ratios=[466.0]), "ratios"),
])
def test_argument_errors_are_raised_without_a_gpu(kwargs, match):
    from sos_amd import tools
    args = dict(signals=[np.zeros(5, np.float32), np.ones(7, np.float64)], noises=[np.zeros(9, np.float32)] * 2, snr=3.0)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        tools.add_signals_ragged(**args)


def test_the_crop_plan_is_the_reference_crop():
    """tools._mix_plan clips noise[start : start + count] to the recording and to the clip like tests/mix_reference.crop."""
    import mix_reference as R
    from sos_amd import tools
    sig = [np.zeros(20, np.float32)] * 6
    noises = [np.zeros(50, np.float32), np.zeros(10, np.float32)]
    index, starts, counts = [0, 0, 0, 0, 1, 1], [0, 40, 50, 60, 3, 0], [20, 20, 20, 20, 100, 0]
    lens, nlens, crop, par, nb = tools._mix_plan(sig, noises, 3.0, index, starts, counts, None, None, 0.5)
    assert lens == [20] * 6 and nlens == [50, 10] and nb == [0] * 6 and np.all(par == [3.0, 0.0])
    for i in range(6):
        assert (int(crop[i, 1]), int(crop[i, 2])) == R.crop(nlens[index[i]], starts[i], counts[i], 20), i
    assert crop[:, 2].tolist() == [20, 10, 0, 0, 7, 0]
