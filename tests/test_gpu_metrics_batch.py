"""metrics.evaluate_metrics_batch (csrc/metrics_batch.hip): a ragged batch of clips scored in one launch sequence.
Per-frame LLR / WSS / frame energies equal the one-clip kernels bit for bit (the frame arithmetic is one copy,
csrc/metrics_frame.h); scalars against the f64 oracle at the tolerances of tests/test_metrics.py; against
evaluate_metrics within 1e-9 relative (a bound on reordered f64 sums of at most 2e5 terms: the sample totals are the only
values whose summation order differs); the same bits alone, in any batch, in any order; the frame count the reference
computes in f64, which is not (n - winlength) // skip."""
import warnings

import numpy as np
import pytest

from oracle import metrics as om
from test_metrics import signals
from util import hashed

pytestmark = pytest.mark.gpu

SR = 16000
KEYS = ["l1", "stoi", "csig", "cbak", "covl", "pesq", "ssnr_regular", "ssnr_shift", "ssnr_clip", "ssnr_exsi", "overall_snr"]
DETAIL_ARRAYS = ["llr", "wss", "energy", "energy_kept"]
DETAIL_COUNTS = ["frames", "kept_samples", "kept_frames"]


def _rel(a, b):
    return abs(float(a) - float(b)) / (abs(float(b)) + 1e-12)


def _same_result(a, b):
    """Two result dicts with the same keys, None in the same places and equal numbers (NaN equal to NaN)."""
    assert list(a) == list(b) == KEYS
    for k in KEYS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(np.float64(a[k]), np.float64(b[k]), equal_nan=True), (k, a[k], b[k])


def _same_detail(a, b):
    for k in DETAIL_COUNTS:
        assert a[k] == b[k], k
    for k in DETAIL_ARRAYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k


def _check_against_oracle(m, clean, noisy, sr, pesq):
    ref = om.composite(clean, noisy, sr, eps=1e-20, pesq_raw=pesq)
    want = dict(l1=om.metrics_L1(noisy, clean),
                ssnr_regular=om.metrics_ssnr(clean, noisy, sr, eps=1e-20)[1],
                ssnr_shift=om.metrics_ssnr_shift(clean, noisy, sr, eps=1e-20)[1],
                ssnr_clip=ref["segSNR"],
                ssnr_exsi=om.metrics_ssnr_exclude_silence(clean, noisy, sr, eps=1e-20)[1],
                overall_snr=ref["overall_snr"], csig=ref["csig"], cbak=ref["cbak"], covl=ref["covl"])
    tol = dict(l1=1e-5, csig=2e-3, cbak=2e-3, covl=2e-3)
    for k, v in want.items():
        err = _rel(m[k], v)
        print(f"  {k:13s} got {m[k]:.9g} oracle {v:.9g} rel {err:.2e}")
        assert err <= tol.get(k, 1e-4), (k, m[k], v)
    assert m["pesq"] == pesq


@pytest.fixture(scope="module")
def ragged():
    """24 clips of 1-10 s at 16 kHz, scored as one batch with a PESQ value supplied."""
    from sos_amd import metrics as M
    lens = np.random.default_rng(31).integers(SR, 10 * SR + 1, size=24)
    pairs = [signals(100 + 2 * i, int(n), SR) for i, n in enumerate(lens)]
    clean, noisy = [p[0] for p in pairs], [p[1] for p in pairs]
    results, detail = M.evaluate_metrics_batch(noisy, clean, sr=SR, pesq=[2.7] * 24, return_detail=True)
    return clean, noisy, results, detail


def test_per_frame_values_are_the_one_clip_kernels_bits(ragged):
    from sos_amd import metrics as M
    clean, noisy, results, detail = ragged
    for c, n, d in zip(clean, noisy, detail):
        l1 = M.llr(c, n, SR)
        w1 = np.asarray(M.wss(c, n, SR, eps=1e-20), dtype=np.float32)
        e1 = M._frame_energies(M._dev(c), M._dev(n), SR)
        assert d["frames"] == len(l1) == int(len(c) / 120 - 4) and d["llr"].dtype == np.float32 and d["wss"].dtype == np.float32
        assert np.array_equal(d["llr"], l1, equal_nan=True)
        assert np.array_equal(d["wss"], w1, equal_nan=True)
        assert d["energy"].dtype == np.float64 and np.array_equal(d["energy"], e1)
        assert d["energy_kept"].shape == (d["kept_frames"], 2) and 0 < d["kept_samples"] <= len(c)


def test_scalars_match_the_f64_oracle(ragged):
    clean, noisy, results, _ = ragged
    for i, (c, n, m) in enumerate(zip(clean, noisy, results)):
        print(f"clip {i} ({len(c)} samples)")
        _check_against_oracle(m, c, n, SR, 2.7)


def test_results_match_evaluate_metrics_clip_by_clip(ragged):
    from sos_amd import metrics as M
    clean, noisy, results, _ = ragged
    plain = M.evaluate_metrics_batch(noisy[:6], clean[:6], sr=SR)
    worst = 0.0
    for i, (c, n, m) in enumerate(zip(clean, noisy, results)):
        for got, pesq in ((m, 2.7),) + (((plain[i], None),) if i < 6 else ()):
            one = M.evaluate_metrics(n, c, sr=SR, pesq=pesq)
            assert list(got) == list(one) == KEYS
            for k in KEYS:
                if one[k] is None:
                    assert got[k] is None, k
                else:
                    worst = max(worst, _rel(got[k], one[k]))
                    assert _rel(got[k], one[k]) <= 1e-9, (i, k, got[k], one[k])
    print(f"largest relative difference to evaluate_metrics: {worst:.2e}")


def test_a_clip_gets_the_same_bits_alone_and_in_any_order(ragged):
    from sos_amd import metrics as M
    clean, noisy, results, detail = ragged
    for i in (0, 7, 23):
        r1, d1 = M.evaluate_metrics_batch([noisy[i]], [clean[i]], sr=SR, pesq=[2.7], return_detail=True)
        _same_result(r1[0], results[i])
        _same_detail(d1[0], detail[i])
    perm = np.random.default_rng(5).permutation(24)
    rp, dp = M.evaluate_metrics_batch([noisy[j] for j in perm], [clean[j] for j in perm], sr=SR, pesq=[2.7] * 24,
                                      return_detail=True)
    for pos, j in enumerate(perm):
        _same_result(rp[pos], results[j])
        _same_detail(dp[pos], detail[j])


def test_chunks_of_a_large_batch_give_the_same_bits(ragged, monkeypatch):
    """More clips than one launch sequence takes (65535) go in chunks; exercised with a chunk size of 5."""
    from sos_amd import metrics as M
    clean, noisy, results, detail = ragged
    monkeypatch.setattr("sos_amd.ragged.MAX_CLIPS", 5)
    rc, dc = M.evaluate_metrics_batch(noisy[:12], clean[:12], sr=SR, pesq=[2.7] * 12, return_detail=True)
    for i in range(12):
        _same_result(rc[i], results[i])
        _same_detail(dc[i], detail[i])


def test_device_table_entries_outside_the_hosts_lengths_are_not_followed():
    """sos_metric_batch called directly: the kernels take offsets and lengths from the device table, and a clip that leaves the
    samples the host's lengths sum to gets status -1 and no work (csrc/ragged.h); the clip before it is scored.  The overrun by
    one sample lies inside the allocation."""
    import ctypes as C
    import torch
    from sos_amd import _lib as L
    from sos_amd import metrics as M
    h = L.lib()
    lens = np.asarray([5000, 9000], dtype=np.int64)
    lp = lens.ctypes.data_as(C.c_void_p)
    buf = torch.zeros(14001, device="cuda")
    tab = torch.tensor([[0, 5000], [5000, 9001]], dtype=torch.int64, device="cuda")         # the second clip overruns
    w, skip, f0, win = M._frame_setup(5000, SR)
    n_fft = 1024
    assert (w, skip, f0, M._frame_setup(9000, SR)[2]) == (480, 120, 37, 71)
    cf = M._crit_filters(SR, n_fft, buf.device)
    need = h.sos_metric_batch_workspace_bytes(lp, 2, w, skip, n_fft)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.zeros(8 * 8 * 2 + 40 * (37 + 71), dtype=torch.uint8, device="cuda")
    assert h.sos_metric_batch(L.ptr(buf), L.ptr(buf), L.ptr(tab[0]), L.ptr(tab[1]), lp, 2, w, skip, n_fft, 16, L.ptr(win), L.ptr(cf),
                              1e-20, L.ptr(ws), need, L.ptr(out), out.numel(), L.stream_ptr()) == 0
    head = np.frombuffer(out.cpu().numpy(), np.float64, 16).reshape(2, 8)
    assert head[0][7] == 0 and head[0][6] == 37 and head[1][7] == -1, head


def test_frame_count_is_the_references_f64_expression():
    """22050 Hz: winlength 662, skip 165.  int(21122 / 165 - 662 / 165) = 123 while (21122 - 662) // 165 = 124."""
    from sos_amd import metrics as M
    sr, k = 22050, 21122
    assert int(k / 165 - (662 / 165)) == 123 and (k - 662) // 165 == 124
    c, n = signals(61, k, sr)
    r, d = M.evaluate_metrics_batch([n], [c], sr=sr, return_detail=True)
    assert d[0]["frames"] == 123 and d[0]["llr"].shape == (123,) and d[0]["energy"].shape == (123, 2)
    # (b) the same count on the device: k samples survive the silence rule, exact zeros follow
    mag = 0.2 + 0.3 * (hashed(62, (k,)) + 1) / 2
    clean = np.zeros(30000)
    clean[:k] = np.where(hashed(63, (k,)) >= 0, 1.0, -1.0) * mag
    noisy = 0.9 * clean + 0.04 * hashed(64, (30000,))
    clean, noisy = clean.astype(np.float32), noisy.astype(np.float32)
    r, d = M.evaluate_metrics_batch([n, noisy], [c, clean], sr=sr, return_detail=True)
    assert d[1]["kept_samples"] == k and d[1]["kept_frames"] == 123 and d[1]["energy_kept"].shape == (123, 2)
    want = om.metrics_ssnr_exclude_silence(clean, noisy, sr, eps=1e-20)[1]
    print(f"ssnr_exsi got {r[1]['ssnr_exsi']:.9g} oracle {want:.9g}")
    assert _rel(r[1]["ssnr_exsi"], want) <= 1e-4


@pytest.mark.parametrize("sr", [8000, 14000])
def test_other_sample_rates_match_the_oracle(sr):
    """8000 Hz: LPC order 10, 240-sample frames under a 512-point transform; 14000 Hz: 420 samples, 1024 points."""
    from sos_amd import metrics as M
    c, n = signals(71, int(2.3 * sr) + 17, sr)
    m = M.evaluate_metrics_batch([n], [c], sr=sr, pesq=[2.7])[0]
    _check_against_oracle(m, c, n, sr, 2.7)


def test_edges_short_clips_and_silence():
    from sos_amd import metrics as M
    lens = [1, 100, 479, 480, 599, 600, 3 * SR]
    pairs = [signals(80 + 2 * i, n, SR) for i, n in enumerate(lens)]
    clean, noisy = [p[0] for p in pairs], [p[1] for p in pairs]
    clean.append(np.zeros(5000, np.float32))                       # an all-zero clean clip among them
    noisy.append(signals(99, 5000, SR)[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # numpy: mean of empty slice, divide by zero
        got, det = M.evaluate_metrics_batch(noisy, clean, sr=SR, return_detail=True)
        alone, det1 = M.evaluate_metrics_batch(noisy[6:7], clean[6:7], sr=SR, return_detail=True)
        _same_result(got[6], alone[0])
        _same_detail(det[6], det1[0])
        for i in range(6):
            _same_result(got[i], M.evaluate_metrics(noisy[i], clean[i], sr=SR))
            assert det[i]["frames"] == (1 if lens[i] == 600 else 0)
            assert np.isnan(got[i]["ssnr_regular"]) == (lens[i] < 600) and np.isfinite(got[i]["l1"])
    assert det[7]["kept_samples"] == 5000 and det[7]["frames"] == 37
    with pytest.raises(ValueError):
        M.evaluate_metrics_batch(noisy[:3], clean[:2], sr=SR)
    with pytest.raises(ValueError):
        M.evaluate_metrics_batch([noisy[6][:-1]], [clean[6]], sr=SR)
    with pytest.raises(ValueError):
        M.evaluate_metrics_batch([noisy[6], np.zeros(0, np.float32)], [clean[6], np.zeros(0, np.float32)], sr=SR)
    with pytest.raises(ValueError):
        M.evaluate_metrics_batch(noisy[:3], clean[:3], sr=SR, pesq=[2.7])


def test_gpu_tensor_inputs_give_the_numpy_inputs_bits():
    import torch
    from sos_amd import metrics as M
    pairs = [signals(120 + 2 * i, n, SR) for i, n in enumerate((20000, 33333, 16001))]
    clean, noisy = [p[0] for p in pairs], [p[1] for p in pairs]
    want, wd = M.evaluate_metrics_batch(noisy, clean, sr=SR, return_detail=True)
    for dtype in (torch.float32, torch.float64):
        tc = [torch.from_numpy(c).cuda().to(dtype) for c in clean]
        tn = [torch.from_numpy(n).cuda().to(dtype) for n in noisy]
        got, gd = M.evaluate_metrics_batch(tn, tc, sr=SR, return_detail=True)
        for a, b, da, db in zip(got, want, gd, wd):
            _same_result(a, b)
            _same_detail(da, db)
    with pytest.raises(RuntimeError):
        M.evaluate_metrics_batch([torch.from_numpy(n) for n in noisy], [torch.from_numpy(c) for c in clean], sr=SR)


def test_stoi_is_computed_for_the_batch_or_passed_through():
    from sos_amd import metrics as M
    pairs = [signals(140 + 2 * i, n, SR) for i, n in enumerate((40000, 52000, 33000))]
    clean, noisy = [p[0] for p in pairs], [p[1] for p in pairs]
    want = M.stoi_batch(clean, noisy, SR)
    got = M.evaluate_metrics_batch(noisy, clean, sr=SR, stoi=True)
    assert [m["stoi"] for m in got] == want and all(0 < s < 1 for s in want)
    given = [0.5, None, "kept as is"]
    got = M.evaluate_metrics_batch(noisy, clean, sr=SR, stoi=given, pesq=[None, 3.1, None])
    assert [m["stoi"] for m in got] == given
    assert [m["pesq"] for m in got] == [None, 3.1, None] and got[0]["csig"] is None and got[1]["csig"] is not None


def _sync_warnings(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in rec)


def test_host_waits_do_not_grow_with_the_batch():
    """One call waits for the device a fixed number of times (the table upload and the one copy back), whatever the
    number of clips; the loop of evaluate_metrics waits about a dozen times per clip."""
    import torch
    from sos_amd import metrics as M
    pairs = [signals(160 + 2 * i, SR + 500 * i, SR) for i in range(64)]
    clean = [torch.from_numpy(p[0]).cuda() for p in pairs]
    noisy = [torch.from_numpy(p[1]).cuda() for p in pairs]
    M.evaluate_metrics_batch(noisy[:2], clean[:2], sr=SR)          # warm-up: code objects, window and filter tables
    w8 = _sync_warnings(lambda: M.evaluate_metrics_batch(noisy[:8], clean[:8], sr=SR))
    w64 = _sync_warnings(lambda: M.evaluate_metrics_batch(noisy, clean, sr=SR))
    loop2 = _sync_warnings(lambda: [M.evaluate_metrics(n, c, sr=SR) for n, c in zip(noisy[:2], clean[:2])])
    loop4 = _sync_warnings(lambda: [M.evaluate_metrics(n, c, sr=SR) for n, c in zip(noisy[:4], clean[:4])])
    print(f"synchronisation warnings: batch of 8: {w8}, batch of 64: {w64}; loop over 2 clips: {loop2}, over 4: {loop4}")
    assert w8 == w64
    assert loop4 > loop2 > w64                                     # the counter counts, and the loop grows with the clips
