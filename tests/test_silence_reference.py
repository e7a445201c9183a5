"""Pins tests/silence_reference.py, the float64 restatement of the silent-interval labeller (sos_amd.labels; CPU only): the
frame rule, the raw decision and the two run-length passes against hand-written expectations; that no input of
tests/test_gpu_labels.py has a frame inside the rounding band around its threshold (which is what lets those tests demand exact
bits); and the host-side validation of the library's two entry points, which touches no device.  Parity with the reference's own
labeller is unpinned (its source is not available)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import silence_reference as R

GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handoff", "dataset_sounds_of_silence.json")


def _bits(plan_string, min_silent=1, min_speech=1, sr=14000, fps=30.0):
    plan = R.plan_from_string(plan_string)
    res = R.label(R.plan_samples(plan, sr, fps, seed=len(plan)), sr, fps, 40.0, min_silent, min_speech)
    assert res["undecided"] == 0 and res["frames"] == len(plan)
    return "".join(str(int(b)) for b in res["bits"])


@pytest.mark.parametrize("sr,fps", R.RATES)
def test_without_the_passes_the_bits_are_the_plan(sr, fps):
    rng = np.random.default_rng(3)
    for F in (1, 2, 7, 64, 301):
        plan = rng.integers(0, 2, size=F).astype(np.uint8)
        plan[0] = 1
        res = R.label(R.plan_samples(plan, sr, fps, seed=F), sr, fps)
        assert np.array_equal(res["bits"], plan) and res["undecided"] == 0
        assert np.allclose(res["energy"], np.where(plan == 1, np.float32(R.LOUD), np.float32(R.QUIET)).astype(np.float64) ** 2,
                           rtol=1e-12, atol=0)
        assert res["silent_frames"] == int((plan == 0).sum())
    quiet_only = R.label(R.plan_samples(np.zeros(9, np.uint8), sr, fps), sr, fps, floor=1e-6)      # the floor decides
    assert not quiet_only["bits"].any() and quiet_only["silent_runs"] == 1
    assert R.label(R.plan_samples(np.zeros(9, np.uint8), sr, fps), sr, fps)["bits"].all()           # all at the maximum: none quiet


# 1 = loud / non-silent, 0 = quiet / silent; minimum run lengths of 3 frames
PASS_ONE = [      # (plan, expected) with min_speech_frames = 3, pass 2 disabled
    ("000 11 000", "000 00 000"),           # a loud run of min - 1 between quiet runs turns quiet
    ("000 111 000", "000 111 000"),         # ... of min stays
    ("11 000 111", "11 000 111"),           # min - 1 touching the start: never changed
    ("111 000 11", "111 000 11"),           # ... touching the end
    ("1 000 1", "1 000 1"),
    ("0 1 0 11 0 111 0", "0 0 0 00 0 111 0"),
    ("11", "11"),
]
PASS_TWO = [      # min_silent_frames = 3, pass 1 disabled
    ("111 00 111", "111 11 111"),           # a quiet run of min - 1 in the interior turns non-quiet
    ("111 000 111", "111 000 111"),         # ... of min stays
    ("00 1111", "11 1111"),                 # min - 1 at the start: changed, wherever it lies
    ("000 1111", "000 1111"),
    ("1111 00", "1111 11"),                 # ... at the end
    ("1111 000", "1111 000"),
    ("1 00 1 00 1", "1 11 1 11 1"),         # each run is judged as it was when the pass began
]


@pytest.mark.parametrize("plan,want", PASS_ONE)
def test_pass_one_by_hand(plan, want):
    assert _bits(plan, 1, 3) == want.replace(" ", "")


@pytest.mark.parametrize("plan,want", PASS_TWO)
def test_pass_two_by_hand(plan, want):
    assert _bits(plan, 3, 1) == want.replace(" ", "")


def test_pass_one_merges_two_quiet_runs_that_pass_two_then_keeps():
    plan = "111 00 1 00 111"
    assert _bits(plan, 4, 2) == "111 00000 111".replace(" ", "")          # 2 + 1 + 2 = 5 >= 4
    assert _bits(plan, 4, 1) == "111 11111 111".replace(" ", "")          # without pass 1 both runs of 2 are too short
    assert _bits(plan, 6, 2) == "111 11111 111".replace(" ", "")          # merged, and still too short
    # unbounded run lengths: a minimum far longer than the clip
    assert _bits("0001000", 1, 10000) == "0000000" and _bits("1110111", 10000, 1) == "1111111"


def test_frame_counts_of_the_golden_json_and_no_empty_frame():
    with open(GOLDEN_JSON) as fp:
        files = json.load(fp)["files"]
    assert [R.frame_count(f["audio_samples"], f["audio_sample_rate"], f["framerate"]) for f in files] == [645, 460]
    assert [f["num_frames"] for f in files] == [645, 460]
    from sos_amd import labels
    for sr, fps in R.RATES:
        ratio = sr / fps
        for n in (1, 2, int(ratio) - 1, int(ratio), int(ratio) + 1, 7777, 120001):
            F = R.frame_count(n, sr, fps)
            lo, hi = R.frame_edges(n, sr, fps)
            assert len(lo) == F and np.all(hi > lo) and lo[0] == 0 and hi[-1] == n and np.all(lo[1:] == hi[:-1]), (sr, fps, n)
            assert labels.frame_count(n, sr, fps) == F                    # the Python layer's count is the contract's
    rng = np.random.default_rng(17)
    for sr, fps in R.RATES:                                               # and over lengths drawn at random, whole frames among them
        for n in list(rng.integers(1, 2_000_000, size=300)) + [int(k * sr / fps) for k in (1, 2, 3, 30, 300, 645)]:
            F = labels.frame_count(int(n), sr, fps)
            assert F == R.frame_count(int(n), sr, fps) and int((F - 1) * (sr / fps)) < n <= int(F * (sr / fps)), (sr, fps, n)


# ---- the inputs of tests/test_gpu_labels.py: none has a frame whose raw decision depends on the summation order
@pytest.mark.parametrize("sr,fps", R.RATES)
def test_no_tile_case_is_undecided(sr, fps):
    for name, plan in R.tile_cases(sr, fps):
        x = R.plan_samples(plan, sr, fps, seed=len(plan))
        res = R.label(x, sr, fps, 40.0, R.MIN_FRAMES, R.MIN_FRAMES)
        assert res["undecided"] == 0 and res["frames"] == len(plan), name
        assert np.array_equal(R.label(x, sr, fps)["bits"], plan), name
    for last in (1, None):                                                # a last frame of one sample; whole frames
        x = R.plan_samples(R.plan_from_string("1101"), sr, fps, seed=4, last_frame_samples=last)
        assert R.label(x, sr, fps)["undecided"] == 0
    ratio = sr / fps
    for n in (1, int(ratio)):
        assert R.label(np.full(n, 0.25, np.float32), sr, fps)["frames"] == 1


def test_no_speechlike_case_is_undecided():
    for x, sr, fps in R.speech_cases():
        for db in (20.0, 40.0):
            res = R.label_seconds(x, sr, fps, db)
            assert res["undecided"] == 0 and 0 < res["silent_frames"] < res["frames"]
    for i, (x, sr, fps) in enumerate(R.batch_cases()):
        assert R.label_seconds(x, sr, fps)["undecided"] == 0, i
    for seed, seconds, sr in ((41, 3.1, 14000), (42, 2.6, 44100), (43, 2.2, 14000)):      # the files of the label_files test
        res = R.label_seconds(R.speechlike(seed, seconds, sr), sr)
        assert res["undecided"] == 0 and 0 < res["silent_frames"] < res["frames"] and res["frames"] >= 60


def test_the_remaining_gpu_inputs_are_not_undecided():
    const = np.where(np.random.default_rng(1).integers(0, 2, size=9000) == 1, 0.2, -0.2).astype(np.float32)
    res = R.label(const, 14000, 30.0)
    assert res["undecided"] == 0 and res["bits"].all()
    for i, p in enumerate(("1101", "10011", "0111")):
        assert R.label(R.plan_samples(R.plan_from_string(p), 14000, 30.0, seed=i), 14000, 30.0)["undecided"] == 0
    # the all-zero clip: E = T = 0 exactly under every summation order (the band's formula counts 0 <= 0 as inside it)
    zero = R.label(np.zeros(9000, np.float32), 14000, 30.0, 40.0, 3)
    assert zero["frames"] == 20 and not zero["bits"].any() and zero["silent_runs"] == 1 and zero["max_energy"] == 0.0


# ---- the library's host-side checks (no GPU: the pointers are dummies and nothing is launched)
def _libs():
    import sos_amd
    from sos_amd import _lib
    out = []
    for mode in ("bf16", "fp16"):
        sos_amd.set_precision(mode)
        out.append(_lib.lib())
    sos_amd.set_precision("bf16")
    return out


def test_both_libraries_export_the_entry_points_and_size_the_workspace():
    tab = np.asarray([[0, 1000, 0, 3], [1000, 467, 3, 2]], dtype=np.int64)
    for h in _libs():
        assert hasattr(h, "sos_silence_label_workspace_bytes") and hasattr(h, "sos_silence_label_batch")
        assert h.sos_abi_version() == 10
        tp = tab.ctypes.data_as(C.c_void_p)
        assert h.sos_silence_label_workspace_bytes(tp, 2) == 256 + 256          # int32 [5] and int32 [5 + 2], 256-byte aligned
        for bad_p, bad_n in ((tp, 0), (tp, 65536), (None, 2)):
            assert h.sos_silence_label_workspace_bytes(bad_p, bad_n) == -1


def _call(h, tab, par, ws_bytes=1 << 20):
    dummy = C.c_void_p(4096)
    return h.sos_silence_label_batch(dummy, dummy, tab.ctypes.data_as(C.c_void_p), len(tab), dummy, par.ctypes.data_as(C.c_void_p),
                                     dummy, ws_bytes, dummy, dummy, dummy, None)


BAD_ENTRIES = [     # (what, column of the table or the parameters of clip 1, value, word of the message)
    ("ratio 1.0", "par", 0, 1.0, "ratio"),
    ("min_silent 0", "par", 3, 0.0, "minimum run lengths"),
    ("min_speech 0.5", "par", 4, 0.5, "minimum run lengths"),
    ("one frame too many", "tab", 3, 4, "the last frame would be empty"),
    ("one frame too few", "tab", 3, 2, "samples would be left over"),
    ("a sample offset past the host total", "tab", 0, 2401, "lies outside"),
    ("a frame offset past the host total", "tab", 2, 4, "lies outside"),
    ("no samples", "tab", 1, 0, "at least 1"),
]


@pytest.mark.parametrize("what,which,col,value,word", BAD_ENTRIES, ids=[b[0] for b in BAD_ENTRIES])
def test_the_launch_refuses_a_bad_entry_by_name_before_touching_the_device(what, which, col, value, word):
    ratio = 14000 / 30.0
    for h in _libs():
        tab = np.asarray([[0, 1000, 0, 3], [1000, 1401, 3, 4]], dtype=np.int64)          # 1401 samples: 3 frames + 1 sample
        par = np.asarray([[ratio, 1e-4, 0.0, 3, 1]] * 2, dtype=np.float64)
        if which == "tab" and col == 3 and value == 4:
            tab[1, 1], value = 1400, 4                                                   # 1400 samples are 3 whole frames
        (tab if which == "tab" else par)[1, col] = value
        assert _call(h, tab, par) == -22, what
        msg = h.sos_last_error().decode()
        assert msg.startswith("sos_silence_label_batch:") and "clip 1" in msg and word in msg, msg


def test_the_launch_refuses_null_pointers_clip_counts_and_a_short_workspace():
    ratio = 14000 / 30.0
    tab = np.asarray([[0, 1000, 0, 3]], dtype=np.int64)
    par = np.asarray([[ratio, 1e-4, 0.0, 3, 1]], dtype=np.float64)
    dummy, tp, pp = C.c_void_p(4096), tab.ctypes.data_as(C.c_void_p), par.ctypes.data_as(C.c_void_p)
    for h in _libs():
        assert h.sos_silence_label_batch(None, dummy, tp, 1, dummy, pp, dummy, 1 << 20, dummy, dummy, dummy, None) == -22
        assert "null" in h.sos_last_error().decode()
        assert h.sos_silence_label_batch(dummy, dummy, tp, 1, dummy, pp, dummy, 1 << 20, None, dummy, dummy, None) == -22
        for bad in (0, 65536):
            assert h.sos_silence_label_batch(dummy, dummy, tp, bad, dummy, pp, dummy, 1 << 20, dummy, dummy, dummy, None) == -22
            assert "65535" in h.sos_last_error().decode()
        need = h.sos_silence_label_workspace_bytes(tp, 1)
        assert _call(h, tab, par, need - 1) == -28 and "workspace" in h.sos_last_error().decode()
