"""SI-SDR / SDR micro-benchmark (run on the GPU box): metrics.si_sdr_batch and metrics.sdr_batch on 256 clean/estimate clip
pairs of 1-10 s at 16 kHz already on the device (the whole call: concatenation, launch sequence, one synchronisation, host
finish), timed with HIP events; the two kernels of the SDR sequence (lag correlations, Levinson solve) timed apart on one
workspace; next to the float64 CPU reference's time per clip (tests/sdr_reference.py) and the largest score difference."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sos_amd  # noqa: E402,F401
from sos_amd import _lib as L  # noqa: E402
from sos_amd import metrics  # noqa: E402
import sdr_reference as R  # noqa: E402
from stoi_reference import closed_form_pair  # noqa: E402


def _timed(fn, iters):
    fn()                                                        # warm-up: code objects
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--filter-length", type=int, default=metrics.SDR_FILTER_LENGTH)
    ap.add_argument("--oracle-clips", type=int, default=8, help="clips the CPU reference scores (time per clip, parity)")
    args = ap.parse_args()
    fs, fl = 16000, args.filter_length
    rng = np.random.default_rng(7)
    lens = rng.integers(1 * fs, 10 * fs + 1, size=args.clips)
    noise = rng.uniform(0.002, 0.5, size=args.clips)
    pairs = [closed_form_pair(1000 + 2 * i, int(n), fs, float(s)) for i, (n, s) in enumerate(zip(lens, noise))]
    xs = [torch.from_numpy(p[0]).cuda() for p in pairs]
    ys = [torch.from_numpy(p[1]).cuda() for p in pairs]
    audio_s = float(lens.sum()) / fs
    print(f"{args.clips} clips, {audio_s:.0f} s of audio at 16 kHz, filter_length {fl}")

    si = metrics.si_sdr_batch(xs, ys)
    sd = metrics.sdr_batch(xs, ys, fl)
    ms_si = _timed(lambda: metrics.si_sdr_batch(xs, ys), args.iters)
    ms_sd = _timed(lambda: metrics.sdr_batch(xs, ys, fl), args.iters)

    # the SDR sequence's two parts on one workspace
    ch = next(metrics._chunks(xs, ys))
    ws = metrics._workspace("sos_sdr_workspace_bytes", ch, fl)
    ms_corr = _timed(lambda: metrics._sdr_enqueue(ch, fl, stages=L.SDR_CORRELATE, ws=ws), args.iters)
    ms_solve = _timed(lambda: metrics._sdr_enqueue(ch, fl, stages=L.SDR_SOLVE, ws=ws), args.iters)
    fma = 2.0 * 512 * float(lens.sum())                        # f64 FMAs of the correlation kernel (it always runs 512 lags)

    t0 = time.perf_counter()
    ref_sd = [R.sdr(*pairs[i], fl) for i in range(args.oracle_clips)]
    cpu_sd = (time.perf_counter() - t0) / max(args.oracle_clips, 1)
    t0 = time.perf_counter()
    ref_si = [R.si_sdr(*pairs[i]) for i in range(args.oracle_clips)]
    cpu_si = (time.perf_counter() - t0) / max(args.oracle_clips, 1)
    err_sd = max([abs(sd[i] - ref_sd[i]) for i in range(args.oracle_clips)] + [0.0])
    err_si = max([abs(si[i] - ref_si[i]) for i in range(args.oracle_clips)] + [0.0])
    print(f"si_sdr_batch {ms_si:8.3f} ms per call ({args.clips / (ms_si / 1e3):9.0f} clips/s); CPU f64 reference "
          f"{cpu_si * 1e3:8.2f} ms per clip; max |GPU - reference| over {args.oracle_clips} clips {err_si:.1e} dB")
    print(f"sdr_batch    {ms_sd:8.3f} ms per call ({args.clips / (ms_sd / 1e3):9.0f} clips/s); CPU f64 reference "
          f"{cpu_sd * 1e3:8.2f} ms per clip; max |GPU - reference| over {args.oracle_clips} clips {err_sd:.1e} dB")
    print(f"  plan + sdr_corr_kernel {ms_corr:8.3f} ms ({2 * fma / (ms_corr / 1e3) / 1e12:6.2f} TFLOP/s f64, workspace "
          f"{ws.numel() / 1e6:.1f} MB); sdr_solve_kernel {ms_solve:8.3f} ms")


if __name__ == "__main__":
    main()
