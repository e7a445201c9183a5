"""sos_resample_batch_f32 (csrc/wave_io.hip): the symbol is part of the C ABI, and its argument checks run on the host
before anything touches the device -- the pointers to device memory below are dummies that are never dereferenced, so no GPU
is needed (the wgrad-tune tests of tests/test_abi_loads.py check host-only validation the same way)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

CHUNK = 4096


def _table(n_in, ratio, n_valid=None):
    n_in = np.asarray(n_in, dtype=np.int64)
    n_out = np.asarray([int(np.ceil(int(n) * ratio)) for n in n_in], dtype=np.int64)
    if n_valid is None:
        n_valid = np.minimum(np.asarray([int(int(n) * ratio) for n in n_in], dtype=np.int64), n_out)
    tiles = -(-n_out // CHUNK)
    return np.ascontiguousarray(np.stack([np.cumsum(n_in) - n_in, n_in, np.cumsum(n_out) - n_out, n_out,
                                          np.asarray(n_valid, dtype=np.int64), np.cumsum(tiles) - tiles]), dtype=np.int64)


def _call(tab, nclips, ratio, nwin=32769, null=None):
    from sos_amd import _lib as L
    h = L.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    args = dict(x=p, table=p, table_host=tab.ctypes.data_as(C.c_void_p), win=p, out=p)
    if null:
        args[null] = C.c_void_p(0)
    rc = h.sos_resample_batch_f32(args["x"], args["table"], args["table_host"], nclips, ratio, args["win"], nwin, 512,
                                  args["out"], None)
    return rc, h.sos_last_error().decode()


def test_symbol_is_declared_in_header_and_bindings():
    from sos_amd import _lib as L
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "sos_hip.h")).read()
    assert re.search(r"\bint\s+sos_resample_batch_f32\s*\(", header)
    assert "sos_resample_batch_f32" in L.SIGNATURES and len(L.SIGNATURES["sos_resample_batch_f32"]) == 10
    m = re.search(r"#define\s+SOS_RESAMPLE_CHUNK\s+(\d+)", header)
    assert m and int(m.group(1)) == L.RESAMPLE_CHUNK == CHUNK
    assert L.lib().sos_abi_version() == 10                       # an added symbol breaks no caller


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_both_library_builds_export_the_symbol(precision):
    import sos_amd
    from sos_amd import _lib as L
    sos_amd.set_precision(precision)
    try:
        assert hasattr(L.lib(), "sos_resample_batch_f32")
    finally:
        sos_amd.set_precision("bf16")


R44 = 14000 / 44100


@pytest.mark.parametrize("tab,nclips,ratio,needle", [
    (_table([700, 800], R44), 0, R44, "clips"),
    (_table([700, 0, 900], R44, n_valid=[222, 0, 285]), 3, R44, "clip 1"),
    (_table([700, 3], R44), 2, R44, "clip 1"),                   # int(3 * 14000 / 44100) = 0 resampled outputs
    (_table([700, 800], R44), 2, 0.0, "ratio"),
], ids=["no-clips", "n_in-0", "n_valid-0", "ratio-0"])
def test_bad_arguments_are_refused_on_the_host(tab, nclips, ratio, needle):
    rc, msg = _call(tab, nclips, ratio)
    assert rc == -22, (rc, msg)                                  # SOS_EINVAL
    assert msg.startswith("sos_resample_batch_f32:") and needle in msg, msg


def test_null_pointers_window_size_and_wrong_lengths_are_refused():
    tab = _table([700, 800], R44)
    for name in ("x", "table", "table_host", "win", "out"):
        rc, msg = _call(tab, 2, R44, null=name)
        assert rc == -22 and "sos_resample_batch_f32: null pointer" in msg, (name, rc, msg)
    rc, msg = _call(tab, 2, R44, nwin=160 * 1024 // 4)           # (nwin + 1) * 4 bytes > 160 KB of LDS
    assert rc == -22 and "LDS" in msg, (rc, msg)
    wrong = _table([700, 800], R44, n_valid=[222, 250])          # int(800 * ratio) = 253
    rc, msg = _call(wrong, 2, R44)
    assert rc == -22 and "clip 1" in msg and "253" in msg, (rc, msg)
    overlap = _table([700, 800], R44)
    overlap[0, 1] = 10                                           # the second clip starts inside the first
    rc, msg = _call(overlap, 2, R44)
    assert rc == -22 and "clip 1" in msg, (rc, msg)
