"""tests/loudness_reference.py against what pins ITU-R BS.1770 / EBU R128 without any meter installed -- the standard's 48 kHz
coefficient table and the EBU Tech 3341 signals with the reading a compliant meter must show -- then the host half of
sos_loudness_batch_f64 / sos_loudness_gain_batch_f32 (csrc/loudness.hip) and the argument checks above them.  Every entry-point
call below is refused on the host before anything is launched: the device pointers are dummies that are never dereferenced, so
no GPU is needed (tests/test_pcm_host_cpu.py does the same for the encode)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import loudness_reference as LR

_buf = (C.c_float * 64)()
P = C.cast(_buf, C.c_void_p)                     # stands for every device pointer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVAIL, CHANNELS, FRAMES, HOPS, SPLIT = [257, 1, 1025], [2, 1, 3], [200, 1, 1100], [80, 80, 110], 8


# ------------------------------------------------------------------------------------------------ the rule
def test_coefficients_at_48_khz_are_the_standards_table():
    from sos_amd import metrics
    assert np.max(np.abs(LR.k_weighting(48000) - LR.TABLE_48K)) < 1e-12
    k = metrics.k_weighting(48000)
    assert k.dtype == np.float64 and k.shape == (10,) and np.max(np.abs(k - LR.TABLE_48K)) < 1e-12
    for sr in (8000, 11025, 44100, 96000):
        assert np.array_equal(metrics.k_weighting(sr), LR.k_weighting(sr))
    assert [metrics.loudness_hop(sr) for sr in (8000, 11025, 44100, 48000)] == [800, 1103, 4410, 4800] == [LR.hop(sr) for sr in (8000, 11025, 44100, 48000)]


def test_the_loop_and_lfilter_are_one_filter():
    rng = np.random.default_rng(5)
    x, k = rng.standard_normal(300), LR.k_weighting(8000)
    saved, LR._lfilter = LR._lfilter, None
    try:
        loop = LR.biquad(k[0:3], np.r_[1.0, k[3:5]], x)
    finally:
        LR._lfilter = saved
    assert np.max(np.abs(loop - LR.biquad(k[0:3], np.r_[1.0, k[3:5]], x))) < 1e-13


@pytest.mark.parametrize("case", sorted(LR.TECH_3341))
def test_tech_3341_readings(case):
    segments, want = LR.TECH_3341[case]
    got = LR.measure(LR.sine(1000.0, 48000, segments, channels=2), 48000)
    print("Tech 3341 case %d: %.4f LUFS (%d of %d blocks)" % (case, got["lufs"], got["blocks"], got["blocks_abs"]))
    assert abs(got["lufs"] - want) <= 0.1


def test_full_scale_997_hz_mono_sine_reads_minus_3_01():
    got = LR.measure(LR.sine(997.0, 48000, [(0.0, 5.0)]), 48000)
    assert abs(got["lufs"] - (-3.01)) <= 0.01 and abs(got["peak"] - 1.0) < 1e-6


def test_short_silent_and_gated_files():
    assert LR.measure(np.ones((1, 4 * 800 - 1), np.float32), 8000) == dict(lufs=-np.inf, peak=1.0, blocks=0, blocks_abs=0, margin=np.inf)
    assert LR.measure(np.zeros((2, 8000), np.float32), 8000)["lufs"] == -np.inf
    quiet_then_loud = LR.sine(1000.0, 8000, [(-60.0, 2.0), (-20.0, 2.0)])
    got = LR.measure(quiet_then_loud, 8000)
    assert got["blocks_abs"] == 37 and 0 < got["blocks"] < got["blocks_abs"]          # the relative gate dropped the quiet half
    padded = LR.measure(quiet_then_loud, 8000, frames=32000 + 8000)                    # zero-filled: 10 more blocks, of which the
    assert padded["blocks_abs"] == 41 and abs(padded["lufs"] - got["lufs"]) < 0.5      # silent ones are gated (3 overlap the sine)
    assert LR.measure(quiet_then_loud, 8000, frames=16000)["lufs"] < -55               # cropped to the quiet half
    assert LR.gain(-np.inf, 0.5, -20.0) == (np.float32(1.0), False) and LR.gain(-30.0, 0.0, -20.0) == (np.float32(1.0), False)
    g, limited = LR.gain(-30.0, 0.5, -20.0, -1.0)                                      # +10 dB would put the peak at +4 dBFS
    assert limited and g == np.float32(10.0 ** (-1.0 / 20.0) / 0.5)
    assert LR.gain(-30.0, 0.1, -20.0, -1.0) == (np.float32(10.0 ** 0.5), False)


# ------------------------------------------------------------------------------------------------ the host half
def _host(a):
    return a.ctypes.data_as(C.c_void_p)


def table():
    from sos_amd import metrics
    return metrics.loudness_table(CHANNELS, AVAIL, FRAMES, HOPS, SPLIT)


def _measure(tab=None, nfiles=3, split=SPLIT, null=None, work_bytes=1 << 30):
    from sos_amd import _lib as L
    tab = table() if tab is None else tab
    a = dict(planes=P, table=P, table_host=_host(tab), coef=P, weights=P, work=P, stats=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_loudness_batch_f64(a["planes"], a["table"], a["table_host"], nfiles, a["coef"], a["weights"], split, a["work"],
                                  work_bytes, a["stats"], None)
    return rc, h.sos_last_error().decode(), "sos_loudness_batch_f64:"


def _gain(tab=None, nfiles=3, null=None, ceiling=-1.0, **_):
    from sos_amd import _lib as L
    tab = table() if tab is None else tab
    a = dict(planes=P, table=P, table_host=_host(tab), stats=P, targets=P, gains=P, limited=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_loudness_gain_batch_f32(a["planes"], a["table"], a["table_host"], nfiles, a["stats"], a["targets"], ceiling, a["gains"],
                                       a["limited"], None)
    return rc, h.sos_last_error().decode(), "sos_loudness_gain_batch_f32:"


def _refused(got, *fragments):
    rc, msg, who = got
    assert rc == -22, (rc, msg)                                  # SOS_EINVAL
    assert msg.startswith(who), msg
    for f in fragments:
        assert f in msg, (f, msg)


def _edit(row, col, value):
    tab = table()
    tab[row, col] = value
    return tab


def test_table_is_the_encode_row_plus_hop_weight_and_chunk():
    tab = table()
    assert tab.dtype == np.int64 and tab.shape == (3, 8)
    assert tab[:, :5].tolist() == [[0, 257, 2, 200, 0], [514, 1, 1, 1, 0], [515, 1025, 3, 1100, 0]]
    assert tab[:, 5:].tolist() == [[80, 0, 0], [80, 2, 2 * 3 * 8], [110, 3, 2 * 3 * 8 + 8]]       # ceil(200 / 80) = 3 hops, 1, 10


def test_header_declares_and_library_exports_the_symbols():
    from sos_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sos_hip.h")).read()
    h = L.lib()
    for name, nargs in (("sos_loudness_batch_f64", 11), ("sos_loudness_gain_batch_f32", 10), ("sos_loudness_workspace_bytes", 3)):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(h, name) and len(L.SIGNATURES[name]) == nargs
    assert h.sos_abi_version() == L.EXPECTED_ABI == 10          # added symbols break no caller
    tab = table()
    chunks = sum(c * -(-f // hop) * SPLIT for c, f, hop in zip(CHANNELS, FRAMES, HOPS))
    assert h.sos_loudness_workspace_bytes(_host(tab), 3, SPLIT) == (chunks * 6 * 8 + 255) // 256 * 256
    assert h.sos_loudness_workspace_bytes(_host(_edit(1, 2, 0)), 3, SPLIT) == -1


@pytest.mark.parametrize("name", ["planes", "table", "table_host", "coef", "weights", "work", "stats"])
def test_measure_refuses_a_null_pointer(name):
    _refused(_measure(null=name), "null pointer")


@pytest.mark.parametrize("name", ["planes", "table", "table_host", "stats", "targets", "gains", "limited"])
def test_gain_refuses_a_null_pointer(name):
    _refused(_gain(null=name), "null pointer")


@pytest.mark.parametrize("call", [_measure, _gain], ids=["measure", "gain"])
def test_file_counts_are_refused(call):
    _refused(call(nfiles=0), "1 .. 65535 files, got 0")
    _refused(call(nfiles=65536), "1 .. 65535 files, got 65536")        # refused before the table is read


def test_split_workspace_and_ceiling_are_refused():
    _refused(_measure(split=0), "1 .. 64 chunks per hop, got 0")
    _refused(_measure(split=65), "1 .. 64 chunks per hop, got 65")
    rc, msg, _ = _measure(work_bytes=1024)
    assert rc == -28 and "the work buffer holds 1024 bytes" in msg      # SOS_ENOSPC
    _refused(_gain(ceiling=0.5), "at most 0 dBFS, got 0.5")
    _refused(_gain(ceiling=float("nan")), "at most 0 dBFS")


@pytest.mark.parametrize("edit,fragments", [
    ((1, 2, 0), ["file 1", "channels outside 1 .. 64"]),
    ((0, 2, 65), ["file 0", "65 channels"]),
    ((2, 1, -5), ["file 2", "-5 available", "negative or too large"]),
    ((0, 3, -1), ["file 0", "-1 frames", "negative or too large"]),
    ((2, 0, 516), ["file 2 (plane sample 516, 1025 available", "outside the totals", "3590 plane samples"]),
    ((1, 0, -1), ["file 1 (plane sample -1", "outside the totals"]),
], ids=["channels=0", "channels=65", "available<0", "frames<0", "planes-past-the-end", "planes<0"])
@pytest.mark.parametrize("call", [_measure, _gain], ids=["measure", "gain"])
def test_both_refuse_one_bad_plane_row_by_file(call, edit, fragments):
    _refused(call(tab=_edit(*edit)), *fragments)


@pytest.mark.parametrize("edit,fragments", [
    ((1, 5, 0), ["file 1", "hop 0", "a hop outside 1 .. 2^31"]),
    ((2, 5, 7), ["file 2", "hop 7", "shorter than the chunks per hop"]),
    ((0, 3, 1 << 59), ["file 0", "negative or too large"]),
    ((2, 6, 4), ["file 2", "weight 4", "outside the totals", "6 channels"]),
    ((1, 6, -1), ["file 1", "weight -1", "outside the totals"]),
    ((2, 7, 57), ["file 2", "chunk 57", "outside the totals", "296 chunks"]),
    ((0, 7, -8), ["file 0", "chunk -8", "outside the totals"]),
], ids=["hop=0", "hop<split", "frames-huge", "weights-past-the-end", "weights<0", "chunks-past-the-end", "chunks<0"])
def test_measure_refuses_one_bad_row_by_file(edit, fragments):
    _refused(_measure(tab=_edit(*edit)), *fragments)


# ------------------------------------------------------------------------------------------------ the argument checks above it
def test_python_argument_errors_are_raised_without_a_gpu():
    import torch
    from sos_amd import audio_io, metrics
    x = torch.zeros(2, 4000)
    with pytest.raises(ValueError, match="file 1 must be"):
        metrics.loudness_batch([x, torch.zeros(4000)], [8000, 8000])
    with pytest.raises(ValueError, match="one rate per file"):
        metrics.loudness_batch([x], [8000, 8000])
    with pytest.raises(ValueError, match="file 0 has the rate 40"):
        metrics.loudness_batch([x], [40])
    with pytest.raises(ValueError, match="file 0 has 2 channels"):
        metrics.loudness_batch([x], [8000], channel_weights=[[1.0, 1.0, 1.0]])
    with pytest.raises(ValueError, match="file 0 has 2 channels"):
        metrics.loudness_batch([x], [8000], channel_weights=[[1.0, -1.0]])
    with pytest.raises(ValueError, match="split is a whole number"):
        metrics.loudness_batch([x], [8000], split=0)
    with pytest.raises(RuntimeError, match="MI355X"):                  # no CPU fallback
        metrics.loudness_batch([x], [8000])
    with pytest.raises(ValueError, match="k_weighting"):
        metrics.k_weighting(0)
    rows = torch.zeros(1, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="one float64 row of 4 per file"):
        audio_io.loudness_gain_batch_device([x], torch.zeros(2, 4, dtype=torch.float64), -20.0)
    with pytest.raises(ValueError, match="finite number of LUFS"):
        audio_io.loudness_gain_batch_device([x], rows, float("nan"))
    with pytest.raises(ValueError, match="at most 0 dBFS"):
        audio_io.loudness_gain_batch_device([x], rows, -20.0, peak_ceiling_db=1.0)
    with pytest.raises(ValueError, match="one float64 per file"):
        audio_io.loudness_gain_batch_device([x], rows, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="MI355X"):
        audio_io.loudness_gain_batch_device([x], rows, -20.0)


@pytest.mark.parametrize("kwargs,match", [
    (dict(loudness=float("nan")), "loudness is None, 'source' or a target within -70 .. 0"),
    (dict(loudness=float("-inf")), "within -70 .. 0"),
    (dict(loudness=-70.5), "within -70 .. 0"),
    (dict(loudness=0.5), "within -70 .. 0"),
    (dict(loudness="loud"), "within -70 .. 0"),
    (dict(loudness=-23.0, peak_ceiling_db=0.1), "at most 0 dBFS"),
    (dict(loudness="source", peak_ceiling_db=float("nan")), "at most 0 dBFS"),
    (dict(loudness=-23.0, channel_weights=[1.0, -0.5]), "finite weights >= 0"),
    (dict(loudness=-23.0, channel_weights={2: [1.0]}), r"channel_weights\[2\] holds 1 weights"),
    (dict(loudness=-23.0, channel_weights=[1.0, 1.0, 1.0]), "2 channels, but channel_weights holds 3 weights"),
])
def test_denoise_recordings_refuses_before_any_launch(kwargs, match, tmp_path):
    """No networks, no device: the call is refused from its arguments and the file's header."""
    import pcm_reference as R
    from sos_amd import recordings
    path = tmp_path / "pair.wav"
    planes = np.zeros((2, 12000), np.float32)
    path.write_bytes(R.container(R.encode(planes, "s16")[0], "s16", 2, 14000))
    with pytest.raises(ValueError, match=match):
        recordings.denoise_recordings(None, None, [str(path)], str(tmp_path / "out"), **kwargs)
    assert not (tmp_path / "out").exists()
