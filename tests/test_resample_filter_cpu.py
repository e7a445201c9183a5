"""The filter rule of the resamplers, one table over the five launch entry points (sos_resample_f32, sos_resample_batch_f32,
sos_resample_merge_batch_f32, sos_stream_resample_f32, sos_stream_band_merge_f32) and the two host-only counts
(sos_stream_resample_ready, sos_stream_band_ready): what each does with a bad ratio, window length or table size.  Every launch
entry point refuses each case on the host before it reads a table or touches a device, so the pointers to device memory and to
the tables are dummies that are never dereferenced and no GPU is needed (tests/test_band_host_cpu.py does the same).  The two
counts run no kernel, so they take a window of any length from 1 entry on; sos_stream_band_ready wants a wing of one sample.
A fragment of the message is asserted where every version of the entry point has told it; the return code and the name always."""
import ctypes as C

import pytest

EINVAL = -22
NWIN, NUM_TABLE = 32769, 512
DOWN, UP = 14000 / 44100, 48000 / 14000       # the band entry points upsample only

_buf = (C.c_int64 * 64)()                     # stands for every device pointer and every table; zeros
P = C.cast(_buf, C.c_void_p)
_i64 = [C.c_int64(0) for _ in range(5)]
REFS = [C.byref(v) for v in _i64]

ENTRIES = {
    "sos_resample_f32": (DOWN, lambda h, r, w, t: h.sos_resample_f32(P, 1000, r, P, w, t, P, 318, None)),
    "sos_resample_batch_f32": (DOWN, lambda h, r, w, t: h.sos_resample_batch_f32(P, P, P, 1, r, P, w, t, P, None)),
    "sos_resample_merge_batch_f32": (UP, lambda h, r, w, t: h.sos_resample_merge_batch_f32(P, P, P, P, P, P, 1, r, P, w, t, 158, P, None)),
    "sos_stream_resample_f32": (DOWN, lambda h, r, w, t: h.sos_stream_resample_f32(P, 2, 8000, P, P, 1, r, P, w, t, P, 64, None)),
    "sos_stream_band_merge_f32": (UP, lambda h, r, w, t: h.sos_stream_band_merge_f32(P, 2, 8000, P, 60, P, P, 1, r, P, w, t, 158, 2, P, 64,
                                                                                      None)),
    "sos_stream_resample_ready": (DOWN, lambda h, r, w, t: h.sos_stream_resample_ready(r, w, t, 1000, *REFS[:2])),
    "sos_stream_band_ready": (UP, lambda h, r, w, t: h.sos_stream_band_ready(r, w, t, 158, 2, 1000, 4000, *REFS)),
}
READY = ("sos_stream_resample_ready", "sos_stream_band_ready")
BAND = ("sos_stream_band_merge_f32", "sos_stream_band_ready")
TELLS_NUM_TABLE = ("sos_stream_resample_f32", "sos_stream_band_merge_f32") + READY

# case -> (what replaces the good argument, the fragment)
CASES = {
    "ratio=0": (dict(ratio=0.0), "ratio=0"),
    "ratio=-1": (dict(ratio=-1.0), "ratio=-1"),
    "ratio=nan": (dict(ratio=float("nan")), "nan"),
    "ratio=1e-4": (dict(ratio=1e-4), "too small for a 512-point table"),
    "nwin=1": (dict(nwin=1), "nwin=1"),
    "nwin=40960": (dict(nwin=40960), "nwin=40960"),       # (nwin + 1) * 4 bytes: one entry more than the 160 KB of LDS hold
    "num_table=0": (dict(num_table=0), "num_table=0"),
}


def _expect(entry, case):
    """-> (return code, fragment or None)"""
    rc, fragment = EINVAL, CASES[case][1]
    if case == "ratio=1e-4" and entry in BAND:
        fragment = "0.0001"                               # no upsampling: refused as a ratio
    if case == "num_table=0" and entry not in TELLS_NUM_TABLE:
        fragment = None
    if entry in READY and case == "nwin=40960":
        rc = 0                                            # no kernel, no LDS to fit
    if entry == "sos_stream_resample_ready" and case == "nwin=1":
        rc = 0                                            # a wing of no sample: every output is final at once
    return rc, (fragment if rc else None)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_filter_rule(entry, case):
    from sos_amd import _lib
    h = _lib.lib()
    good, call = ENTRIES[entry]
    a = dict(dict(ratio=good, nwin=NWIN, num_table=NUM_TABLE), **CASES[case][0])
    want, fragment = _expect(entry, case)
    rc = call(h, a["ratio"], a["nwin"], a["num_table"])
    msg = h.sos_last_error().decode()
    assert rc == want, (rc, msg)
    if want:
        assert msg.startswith(entry + ":"), msg
    if fragment:
        assert fragment in msg, (fragment, msg)


@pytest.mark.parametrize("entry", READY)
def test_the_good_arguments_of_the_table_are_accepted_where_no_device_is_needed(entry):
    from sos_amd import _lib
    h = _lib.lib()
    good, call = ENTRIES[entry]
    assert call(h, good, NWIN, NUM_TABLE) == 0, h.sos_last_error()
    assert _i64[0].value > 0
